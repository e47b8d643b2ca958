// gfx950 (CDNA4) kernels for the batched NN evaluation path -- layer-granular set.
// One workgroup = one board (64 squares = the GEMM's N dimension), 4 waves of 64 lanes; dense convolutions are
// implicit GEMMs on MFMA with the board tile staged in LDS, depthwise / SE / heads run on the VALU.
//
// Reference semantics implemented here (file:line relative to /root/reference):
//   conv+BN(+ReLU) stacks ........ DeepCrazyhouse/src/domain/neural_net/architectures/pytorch/builder_util.py:154-178,437-475
//   SE gates ...................... builder_util.py:49-114
//   policy / value heads .......... builder_util.py:206-326
//   softmax on policy_out ......... engine/src/nn/tensorrtapi.cpp:378-392, engine/src/nn/neuralnetapi.cpp:241-260
#include "kernels.h"

#include <algorithm>
#include <stdexcept>
#include "device_utils.h"
#include "value_head_body.h"

namespace cra {


// ================================================================================================================
// Dense conv (1x1 / 3x3, pad k/2) as implicit GEMM:  D[cout][square] = sum_{tap,ci} W[cout][tap][ci] * X[nbr(square,tap)][ci]
// A operand = packed weight fragment straight from L2 (1 KiB contiguous per wave), B operand = board rows from LDS
// (row 64 is a zero row that out-of-board taps point at).  Each wave owns 16 couts x 64 squares (4 accumulators);
// D's lane layout (col = square = lane&15, rows = 4 consecutive couts) gives 8/16-byte NHWC stores.
// ================================================================================================================
template <typename T, int KS>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const ConvArgs a) {
    using frag = typename VT<T>::frag;
    constexpr int KC = VT<T>::KC;
    constexpr int ROWP = KC + 16 / int(sizeof(T));   // +16 B per row: consecutive rows land on different bank groups
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs = reinterpret_cast<T*>(smem);               // [65][ROWP]

    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int l15 = lane & 15, lg = lane >> 4;
    const int co_tile = blockIdx.x * 4 + wave;
    const bool active = co_tile * 16 < a.cout_pad;
    const int x_ld = a.x_ld ? a.x_ld : a.cin;
    const T* xb = reinterpret_cast<const T*>(a.x) + size_t(b) * kSquares * x_ld;
    const int nslab_ci = a.cin >> 5;
    const int nslab = KS * KS * nslab_ci;
    const frag* wp = reinterpret_cast<const frag*>(a.wpk) + size_t(active ? co_tile : 0) * nslab * 64 + lane;

    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int i = tid; i < ROWP; i += 256) xs[64 * ROWP + i] = T(0);

    for (int kc0 = 0; kc0 < a.cin; kc0 += KC) {
        const int kcl = min(KC, a.cin - kc0);
        __syncthreads();
        const int vec_per_row = kcl * int(sizeof(T)) / 16;
        for (int i = tid; i < kSquares * vec_per_row; i += 256) {
            const int r = i / vec_per_row, v = i - r * vec_per_row;
            const uint4 d = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(xb + size_t(r) * x_ld + kc0) + v * 16);
            *reinterpret_cast<uint4*>(reinterpret_cast<char*>(xs + r * ROWP) + v * 16) = d;
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int tap = 0; tap < KS * KS; ++tap) {
                const int dy = tap / KS - KS / 2, dx = tap % KS - KS / 2;
                int rowoff[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int sq = t * 16 + l15;
                    const int ny = (sq >> 3) + dy, nx = (sq & 7) + dx;
                    const bool ok = (unsigned(ny) < 8u) && (unsigned(nx) < 8u);
                    rowoff[t] = (ok ? ny * 8 + nx : 64) * ROWP + lg * 8;
                }
                const frag* wps = wp + size_t(tap * nslab_ci + (kc0 >> 5)) * 64;
                const int ns = kcl >> 5;
                for (int sl = 0; sl < ns; ++sl) {
                    const frag af = wps[size_t(sl) * 64];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const frag bf = *reinterpret_cast<const frag*>(xs + rowoff[t] + sl * 32);
                        mma_k32(af, bf, acc[t]);
                    }
                }
            }
        }
    }
    if (!active) return;

    const int co0 = co_tile * 16 + lg * 4;
    float bs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bs[r] = a.bias[co0 + r];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int sq = t * 16 + l15;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[t][r] + bs[r];
        if (a.relu == 2) {                           // activation is the body's last module, the shortcut is added after it
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if (a.resid) {
            float rv[4];
            load4<T>(reinterpret_cast<const T*>(a.resid) + (size_t(b) * kSquares + sq) * a.cout_ld + co0, rv);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += rv[r];
        }
        if (a.relu == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if (a.out_policy_f32) {
            float* o = reinterpret_cast<float*>(a.out) + size_t(b) * a.cout_real * kSquares;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (co0 + r < a.cout_real) o[(co0 + r) * kSquares + sq] = v[r];
        } else if (a.out_rows_f32) {                 // FC over the batch: row = board, float logits [rows_valid][cout_real]
            const int row = b * kSquares + sq;
            if (row < a.rows_valid) {
                float* o = reinterpret_cast<float*>(a.out) + size_t(row) * a.cout_real;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co0 + r < a.cout_real) o[co0 + r] = v[r];
            }
        } else if (a.out_flat) {
            T* o = reinterpret_cast<T*>(a.out) + size_t(b) * a.flat_pitch;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (co0 + r < a.cout_real) o[(co0 + r) * kSquares + sq] = T(v[r]);
        } else {
            store4<T>(reinterpret_cast<T*>(a.out) + (size_t(b) * kSquares + sq) * a.cout_ld + co0, v);
        }
    }
}

template <typename T> void launch_conv_gemm(const ConvArgs& a, hipStream_t s) {
    constexpr int KC = VT<T>::KC;
    constexpr int ROWP = KC + 16 / int(sizeof(T));
    const size_t shmem = size_t(65) * ROWP * sizeof(T);
    dim3 grid((a.cout_pad + 63) / 64, a.batch), block(256);
    if (a.ks == 1) hipLaunchKernelGGL((conv_gemm_kernel<T, 1>), grid, block, shmem, s, a);
    else hipLaunchKernelGGL((conv_gemm_kernel<T, 3>), grid, block, shmem, s, a);
}
template void launch_conv_gemm<half_t>(const ConvArgs&, hipStream_t);
template void launch_conv_gemm<float>(const ConvArgs&, hipStream_t);

// ================================================================================================================
// Depthwise k x k + folded BN + ReLU (VALU, fp32 accumulate).  grid (C/32, B); thread = 8 channels x 1 square.
// ================================================================================================================
template <typename T, int KS>
__global__ __launch_bounds__(256) void depthwise_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                        const float* __restrict__ w, const float* __restrict__ bias, int C) {
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * 32 + (threadIdx.x & 3) * 8;
    const int sq = threadIdx.x >> 2;
    const int py = sq >> 3, px = sq & 7;
    const T* xb = x + size_t(b) * kSquares * C;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bias[c0 + j];
#pragma unroll
    for (int tap = 0; tap < KS * KS; ++tap) {
        const int ny = py + tap / KS - KS / 2, nx = px + tap % KS - KS / 2;
        if ((unsigned(ny) < 8u) && (unsigned(nx) < 8u)) {
            float xv[8], wv[8];
            load8<T>(xb + size_t(ny * 8 + nx) * C + c0, xv);
            load8<float>(w + size_t(tap) * C + c0, wv);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(wv[j], xv[j], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaxf(acc[j], 0.f);
    store8<T>(y + (size_t(b) * kSquares + sq) * C + c0, acc);
}

template <typename T>
void launch_depthwise(const T* x, T* y, const float* w, const float* bias, int batch, int C, int ks, hipStream_t s) {
    dim3 grid(C / 32, batch), block(256);
    if (ks == 3) hipLaunchKernelGGL((depthwise_kernel<T, 3>), grid, block, 0, s, x, y, w, bias, C);
    else hipLaunchKernelGGL((depthwise_kernel<T, 5>), grid, block, 0, s, x, y, w, bias, C);
}
template void launch_depthwise<half_t>(const half_t*, half_t*, const float*, const float*, int, int, int, hipStream_t);
template void launch_depthwise<float>(const float*, float*, const float*, const float*, int, int, int, hipStream_t);

// ================================================================================================================
// Squeeze-excitation gate, in place.  One workgroup per board.
// ================================================================================================================

// kind: 1 ca_se / se (two bias-free FCs), 2 eca_se (centre-tap linear + bias); + 16 = plain sigmoid instead of hard-sigmoid
// (AlphaZero's ResidualBlock builds its gate with use_hard_sigmoid=False, a0_resnet.py:95).  res != nullptr: the gated tensor is the
// body of a residual block and the shortcut is added here: x = relu(res + x * gate) (a0_resnet.py:104-107).
template <typename T>
__global__ __launch_bounds__(256) void se_kernel(T* __restrict__ x, int kind_flags, const float* __restrict__ w1t,
                                                 const float* __restrict__ w2t, const float* __restrict__ b1, int C,
                                                 const T* __restrict__ res) {
    const int kind = kind_flags & 15;
    const bool plain_sigmoid = (kind_flags & 16) != 0;
    auto gate_act = [&](float v) { return plain_sigmoid ? 1.f / (1.f + expf(-v)) : hard_sigmoid(v); };
    __shared__ float s_mean[512];
    __shared__ float s_h[512];
    __shared__ float s_y[512];
    const int tid = threadIdx.x;
    T* xb = x + size_t(blockIdx.x) * kSquares * C;
    for (int c = tid; c < C; c += 256) {
        float sum = 0.f;
        for (int sq = 0; sq < kSquares; ++sq) sum += to_f(xb[size_t(sq) * C + c]);
        s_mean[c] = sum * (1.f / 64.f);
    }
    __syncthreads();
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
            s_y[c] = gate_act(sum);
        }
    } else {
        for (int c = tid; c < C; c += 256) {
            float sum = b1[c];
            for (int i = 0; i < C; ++i) sum = fmaf(w1t[size_t(i) * C + c], s_mean[i], sum);
            s_y[c] = gate_act(sum);
        }
    }
    __syncthreads();
    const int nvec = kSquares * C / 8;
    const T* rb = res ? res + size_t(blockIdx.x) * kSquares * C : nullptr;
    for (int i = tid; i < nvec; i += 256) {
        const int c0 = (i * 8) % C;
        float v[8];
        load8<T>(xb + size_t(i) * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= s_y[c0 + j];
        if (rb) {
            float r[8];
            load8<T>(rb + size_t(i) * 8, r);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j] + r[j], 0.f);
        }
        store8<T>(xb + size_t(i) * 8, v);
    }
}

// ---- SE gate on pooled sums: 8 boards per 1024-thread workgroup -------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(1024) void se_gate_kernel(const float* __restrict__ pool, float* __restrict__ gate,
                                                       const float* __restrict__ w1t, const float* __restrict__ w2t,
                                                       const float* __restrict__ b1, int batch) {
    constexpr int C = 256, H = 128, NB = 8;
    __shared__ float s_mean[NB][C];            //  8 KB
    __shared__ float s_part[8 * NB * H];       // 32 KB (also reused as [4][NB][C])
    __shared__ float s_h[NB][H];               //  4 KB
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * NB;
    const int nb = min(NB, batch - b0);
    for (int i = tid; i < NB * C; i += 1024) {
        const int bb = i / C, c = i - bb * C;
        s_mean[bb][c] = bb < nb ? pool[size_t(b0 + bb) * C + c] * (1.f / 64.f) : 0.f;
    }
    __syncthreads();
    if (KIND == 1) {
        {   // FC1: 128 outputs, K = 256 split in 8 slices of 32
            const int j = tid & (H - 1), kq = tid >> 7;
            float w[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) w[k] = w1t[size_t(kq * 32 + k) * H + j];
            float acc[NB];
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) acc[bb] = 0.f;
#pragma unroll
            for (int k = 0; k < 32; ++k)
#pragma unroll
                for (int bb = 0; bb < NB; ++bb) acc[bb] = fmaf(w[k], s_mean[bb][kq * 32 + k], acc[bb]);
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) s_part[(kq * NB + bb) * H + j] = acc[bb];
        }
        __syncthreads();
        {
            const int bb = tid >> 7, j = tid & (H - 1);
            float sum = 0.f;
#pragma unroll
            for (int kq = 0; kq < 8; ++kq) sum += s_part[(kq * NB + bb) * H + j];
            s_h[bb][j] = fmaxf(sum, 0.f);
        }
        __syncthreads();
        {   // FC2: 256 outputs, K = 128 split in 4 slices of 32
            const int c = tid & (C - 1), kq = tid >> 8;
            float w[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) w[k] = w2t[size_t(kq * 32 + k) * C + c];
            float acc[NB];
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) acc[bb] = 0.f;
#pragma unroll
            for (int k = 0; k < 32; ++k)
#pragma unroll
                for (int bb = 0; bb < NB; ++bb) acc[bb] = fmaf(w[k], s_h[bb][kq * 32 + k], acc[bb]);
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) s_part[(kq * NB + bb) * C + c] = acc[bb];
        }
    } else {
        // eca: 256 outputs, K = 256 split in 4 slices of 64
        const int c = tid & (C - 1), kq = tid >> 8;
        float acc[NB];
#pragma unroll
        for (int bb = 0; bb < NB; ++bb) acc[bb] = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float w[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) w[k] = w1t[size_t(kq * 64 + h * 32 + k) * C + c];
#pragma unroll
            for (int k = 0; k < 32; ++k)
#pragma unroll
                for (int bb = 0; bb < NB; ++bb) acc[bb] = fmaf(w[k], s_mean[bb][kq * 64 + h * 32 + k], acc[bb]);
        }
#pragma unroll
        for (int bb = 0; bb < NB; ++bb) s_part[(kq * NB + bb) * C + c] = acc[bb];
    }
    __syncthreads();
    for (int i = tid; i < NB * C; i += 1024) {
        const int bb = i / C, c = i - bb * C;
        if (bb < nb) {
            float sum = KIND == 2 ? b1[c] : 0.f;
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) sum += s_part[(kq * NB + bb) * C + c];
            gate[size_t(b0 + bb) * C + c] = hard_sigmoid(sum);
        }
    }
}

void launch_se_gate(const float* pool, float* gate, int kind, const float* w1t, const float* w2t, const float* b1, int batch, int C,
                    hipStream_t s) {
    (void)C;   // specialised for C = 256 (checked by the caller)
    dim3 grid((batch + 7) / 8), block(1024);
    if (kind == 1) hipLaunchKernelGGL(se_gate_kernel<1>, grid, block, 0, s, pool, gate, w1t, w2t, b1, batch);
    else hipLaunchKernelGGL(se_gate_kernel<2>, grid, block, 0, s, pool, gate, w1t, w2t, b1, batch);
}

template <typename T>
void launch_se(T* x, int kind_flags, const float* w1t, const float* w2t, const float* b1, int batch, int C, hipStream_t s, const T* res) {
    hipLaunchKernelGGL((se_kernel<T>), dim3(batch), dim3(256), 0, s, x, kind_flags, w1t, w2t, b1, C, res);
}
template void launch_se<half_t>(half_t*, int, const float*, const float*, const float*, int, int, hipStream_t, const half_t*);
template void launch_se<float>(float*, int, const float*, const float*, const float*, int, int, hipStream_t, const float*);

// ================================================================================================================
// Value head: conv1x1(C->cv)+BN+ReLU -> channel-major flatten -> FC(fc)+ReLU -> FC(1) -> tanh
//             or (WDLP) FC(3) / FC(1)+sigmoid, value = -softmax(wdl)[0] + softmax(wdl)[2], aux = [wdl, plys].
// ================================================================================================================

// The whole value head of one board in exact f32 on the vector units (0.5 MFLOP per board: the cost is moving the board, not the
// arithmetic).  The board tile is staged once (coalesced) with the folded conv weights beside it; conv 1x1: thread = (square, group of
// channels), a 16-byte LDS read of the square's row per four input channels, the weights as broadcast reads; FC1: thread = (four outputs, a quarter
// of the inputs), a row of the transposed weight matrix as one 16-byte load per lane, 32 loads in flight.  Precision float16x3 runs this kernel (one launch instead of conv
// GEMM + FC GEMM + final), as do the unfused layer paths.
//
// PROBE (development, ValueHeadArgs::variant & 16, needs dbg): the instantiation round 5's root-cause harness launches
// (scripts/value_head_rootcause.py).  Behind the launch's [B][8 + 1024] checksum area it leaves, per board, 16 words of header (words 0-3:
// HW_ID of waves 0-3, word 4: XCC_ID) and three more [1024]-word images in s_part's layout: (1) the FC1 sums read back from LDS right
// behind the barrier, (2) the SAME sums stored to global memory straight from the accumulator registers, never through LDS, (3) integer
// checksums of the 16-byte weight loads per lane and component (sum of the loaded words' bit patterns) -- so that a differing launch says
// whether the loaded words, the accumulator register or only its way through LDS was wrong.
//
// SCALAR_FMA (the product form): FC1's products as four v_fmac_f32 per weight row, written out, instead of the two v_pk_fma_f32 the
// compiler makes of them.  Round 5's root cause of the "value head's compute unit" (profiles/NOTES.md): the words that came out wrong
// were always the LOW halves of v_pk_fma_f32 results in lanes 48-63, beside a neighbour workgroup that issues MFMAs on the same SIMD --
// 8,401 of 10,000 launches with the packed form, 0 of 10,000 with this one, same co-residency.  The whole library is built without
// packed f32 arithmetic since (crazyara_amd/build.py); the asm pins this kernel's form whatever the build says.  variant & 32 brings the
// packed form back (the harness's positive control, meaningful only in a CRA_BUILD_PACKED_FP32 build).
template <typename T, bool PROBE = false, bool SCALAR_FMA = false>
__global__ __launch_bounds__(256) void value_head_kernel(const ValueHeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    value_head_body<T, PROBE, SCALAR_FMA>(a, smem, blockIdx.x);     // value_head_body.h
}
template <typename T>
__global__ __launch_bounds__(512) void value_head_kernel_8w(const ValueHeadArgs a) {      // the product form on eight waves
    extern __shared__ __attribute__((aligned(16))) char smem[];
    value_head_body<T, false, true, 512>(a, smem, blockIdx.x);
}

template <typename T>
__global__ __launch_bounds__(256) void value_final_kernel(const ValueFinalArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + wave;
    if (b >= a.batch) return;
    const T* in = reinterpret_cast<const T*>(a.in) + size_t(b) * a.n;
    if (!a.wdlp) {
        float part = 0.f;
        for (int i = lane; i < a.n; i += 64) part = fmaf(a.w[i], to_f(in[i]), part);
        part = wave_sum(part);
        if (lane == 0) a.value[b] = tanhf(part + a.b[0]);
        return;
    }
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < a.n; i += 64) {
        const float f = to_f(in[i]);
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = fmaf(a.w[k * a.n + i], f, p[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = wave_sum(p[k]);
    if (lane == 0) {
        const float l0 = p[0] + a.b[0], l1 = p[1] + a.b[1], l2 = p[2] + a.b[2];
        const float m = fmaxf(l0, fmaxf(l1, l2));
        const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m);
        const float inv = 1.f / (e0 + e1 + e2);
        a.value[b] = -e0 * inv + e2 * inv;
        if (a.aux) {
            a.aux[b * 4 + 0] = l0;
            a.aux[b * 4 + 1] = l1;
            a.aux[b * 4 + 2] = l2;
            a.aux[b * 4 + 3] = 1.f / (1.f + expf(-(p[3] + a.b[3])));
        }
    }
}

template <typename T> void launch_value_final(const ValueFinalArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((value_final_kernel<T>), dim3((a.batch + 3) / 4), dim3(256), 0, s, a);
}
template void launch_value_final<half_t>(const ValueFinalArgs&, hipStream_t);
template void launch_value_final<float>(const ValueFinalArgs&, hipStream_t);

// Round 4 made this kernel ask for (nearly) a whole compute unit's LDS: with workgroups of the float16x3 policy conv
// (conv_gemm_x3_kernel<3, 1, 8, 4>) on the same compute unit, one FC1 accumulator came out wrong in lanes 48-63 of one wave in 20-80 % of
// the launches, cause unknown.  Round 5 found the cause (profiles/NOTES.md): the accumulator was the low half of a v_pk_fma_f32 result, and
// v_pk_fma_f32 goes wrong beside a wave of another workgroup that issues MFMAs on the same SIMD (standalone reproducer:
// scripts/ubench/neighbour_mfma.hip).  FC1 now runs on v_fmac_f32 (SCALAR_FMA above) and the library holds no packed f32 arithmetic
// (crazyara_amd/build.py), after which every (victim, aggressor) pair of ops of the conformant forwards is clean WITHOUT the fence
// (scripts/coresidency_screen.py, profiles/r05/).  The fence is therefore off; lds_pad >= 0 (CRA_VALUE_HEAD_LDS_PAD=0) brings it back.
constexpr size_t kValueHeadExclusiveLds = 144 * 1024;
size_t value_head_lds_bytes(const ValueHeadArgs& a) {
    const size_t used = (size_t(kSquares) * (a.C / 2 + 4) + size_t(a.cv) * a.C + size_t(kSquares) * a.cv + 8 + ((a.variant & 1) ? 4 * a.fc : 0)) * sizeof(float);
    if (a.lds_pad < 0) return used;                              // development: the kernel as it was (shares compute units)
    return std::max(used + size_t(a.lds_pad), kValueHeadExclusiveLds);
}
// the product form (no debug record, FC1 on v_fmac_f32, partial sums over the dead board tile) runs on eight waves; variant & 64: on four (A/B)
static bool value_head_eight_waves(const ValueHeadArgs& a) { return !a.dbg && (a.variant & (1 | 16 | 32 | 64)) == 0; }
template <typename T> const void* value_head_function(const ValueHeadArgs& a) {        // the instantiation launch_value_head picks
    if (value_head_eight_waves(a)) return reinterpret_cast<const void*>(&value_head_kernel_8w<T>);
    const bool probe = a.dbg && (a.variant & 16), scalar = (a.variant & 32) == 0;
    if (probe && scalar) return reinterpret_cast<const void*>(&value_head_kernel<T, true, true>);
    if (probe) return reinterpret_cast<const void*>(&value_head_kernel<T, true, false>);
    if (scalar) return reinterpret_cast<const void*>(&value_head_kernel<T, false, true>);
    return reinterpret_cast<const void*>(&value_head_kernel<T, false, false>);
}
// once per net, outside any stream capture: the kernel's dynamic LDS allowance (the staged board is more than the default 64 KiB)
template <typename T> void prepare_value_head(const ValueHeadArgs& a) {
    if (a.C % 16 != 0 || a.cv > 16 || (!a.wwdl && a.fc % 4 != 0)) throw std::runtime_error("value head: channels must be a multiple of 16, value channels at most 16, FC width a multiple of 4");
    const size_t shmem = value_head_lds_bytes(a);
    if (shmem > 160 * 1024) throw std::runtime_error("value head: the board tile does not fit the LDS");
    // per net build, like the other kernels' allowances: the attribute belongs to the current DEVICE's copy of the function, so a
    // remembered process-wide maximum would leave the second device of a First/Last_Device_ID range at the default 64 KiB
    if (shmem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(value_head_function<T>(a), hipFuncAttributeMaxDynamicSharedMemorySize, int(shmem));
        if (e != hipSuccess) throw std::runtime_error(std::string("value head: hipFuncSetAttribute failed: ") + hipGetErrorString(e));
    }
}
template void prepare_value_head<half_t>(const ValueHeadArgs&);
template void prepare_value_head<float>(const ValueHeadArgs&);
template <typename T> void launch_value_head(const ValueHeadArgs& a, hipStream_t s) {
    const bool probe = a.dbg && (a.variant & 16), scalar = (a.variant & 32) == 0;
    if (value_head_eight_waves(a)) {
        hipLaunchKernelGGL((value_head_kernel_8w<T>), dim3(a.batch), dim3(512), value_head_lds_bytes(a), s, a);
        return;
    }
    if (probe && scalar) hipLaunchKernelGGL((value_head_kernel<T, true, true>), dim3(a.batch), dim3(256), value_head_lds_bytes(a), s, a);
    else if (probe) hipLaunchKernelGGL((value_head_kernel<T, true, false>), dim3(a.batch), dim3(256), value_head_lds_bytes(a), s, a);
    else if (scalar) hipLaunchKernelGGL((value_head_kernel<T, false, true>), dim3(a.batch), dim3(256), value_head_lds_bytes(a), s, a);
    else hipLaunchKernelGGL((value_head_kernel<T, false, false>), dim3(a.batch), dim3(256), value_head_lds_bytes(a), s, a);
}
template void launch_value_head<half_t>(const ValueHeadArgs&, hipStream_t);
template void launch_value_head<float>(const ValueHeadArgs&, hipStream_t);

// ================================================================================================================
// Row softmax (policy_softmax output of the reference's GPU backend).
// ================================================================================================================
__global__ __launch_bounds__(256) void softmax_kernel(const float* __restrict__ logits, float* __restrict__ probs, int n) {
    __shared__ float s_red[4];
    const float* in = logits + size_t(blockIdx.x) * n;
    float* out = probs + size_t(blockIdx.x) * n;
    const int tid = threadIdx.x;
    float m = -INFINITY;
    for (int i = tid; i < n; i += 256) m = fmaxf(m, in[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) s_red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    float sum = 0.f;
    for (int i = tid; i < n; i += 256) sum += expf(in[i] - m);
    sum = block_sum_256(sum, s_red);
    const float c = m + logf(sum);   // exp(x - (max + log(sum))) as in apply_softmax(), neuralnetapi.cpp:241-260
    for (int i = tid; i < n; i += 256) out[i] = expf(in[i] - c);
}

// one workgroup per slot; a slot has at most `stride` entries, the reads hit the row of probabilities the forward just wrote;
// the last workgroup carries the values (and aux) of the whole batch
__global__ void gather_probs_kernel(const float* __restrict__ probs, int nb_policy, const uint16_t* __restrict__ idx,
                                    const uint32_t* __restrict__ cnt, int stride, int n_slots, float* __restrict__ out,
                                    const float* __restrict__ value_dev, float* __restrict__ value_out, int batch,
                                    const float* __restrict__ aux_dev, float* __restrict__ aux_out) {
    const int slot = blockIdx.x;
    if (slot == n_slots) {
        for (int i = threadIdx.x; i < batch; i += blockDim.x) value_out[i] = value_dev[i];
        if (aux_dev != nullptr)
            for (int i = threadIdx.x; i < batch * 4; i += blockDim.x) aux_out[i] = aux_dev[i];
        return;
    }
    const uint32_t n = cnt[slot];
    const float* row = probs + size_t(slot) * nb_policy;
    const size_t base = size_t(slot) * stride;
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) out[base + j] = row[idx[base + j]];
}

void launch_gather_probs(const float* probs, int nb_policy, const uint16_t* idx, const uint32_t* cnt, int stride, int n_slots, float* out,
                         const float* value_dev, float* value_out, int batch, const float* aux_dev, float* aux_out, hipStream_t s) {
    hipLaunchKernelGGL(gather_probs_kernel, dim3(n_slots + 1), dim3(64), 0, s, probs, nb_policy, idx, cnt, stride, n_slots, out, value_dev,
                       value_out, batch, aux_dev, aux_out);
}

// ---- routed batches (an expert set, rise_net.hip): an expert ran its group packed (slot w = board board_of[w] of the batch) ----
// gather_probs_kernel for a group: slot w's priors, value and aux go to board board_of[w]'s places in the caller's buffers, read through
// that board's index list
__global__ void gather_probs_indexed_kernel(const float* __restrict__ probs, int nb_policy, const uint16_t* __restrict__ idx,
                                            const uint32_t* __restrict__ cnt, int stride, const int* __restrict__ board_of,
                                            float* __restrict__ out, const float* __restrict__ value_dev, float* __restrict__ value_out,
                                            const float* __restrict__ aux_dev, float* __restrict__ aux_out) {
    const int w = blockIdx.x;
    const int board = board_of[w];
    if (threadIdx.x == 0) value_out[board] = value_dev[w];
    if (aux_dev != nullptr && threadIdx.x < 4) aux_out[board * 4 + threadIdx.x] = aux_dev[w * 4 + threadIdx.x];
    const uint32_t n = min(cnt[board], uint32_t(stride));
    const float* row = probs + size_t(w) * nb_policy;
    const size_t base = size_t(board) * stride;
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) out[base + j] = row[idx[base + j]];
}
void launch_gather_probs_indexed(const float* probs, int nb_policy, const uint16_t* idx, const uint32_t* cnt, int stride, const int* board_of,
                                 int n_slots, float* out, const float* value_dev, float* value_out, const float* aux_dev, float* aux_out,
                                 hipStream_t s) {
    hipLaunchKernelGGL(gather_probs_indexed_kernel, dim3(n_slots), dim3(64), 0, s, probs, nb_policy, idx, cnt, stride, board_of, out, value_dev,
                       value_out, aux_dev, aux_out);
}

// whole rows of a group into the batch's tensors: dst row board_of[w] = src row w (probabilities, optionally logits; value and aux ride along)
__global__ __launch_bounds__(256) void scatter_rows_indexed_kernel(const float* __restrict__ probs, const float* __restrict__ logits, int nb_policy,
                                                                   const int* __restrict__ board_of, float* __restrict__ probs_out,
                                                                   float* __restrict__ logits_out, const float* __restrict__ value_dev,
                                                                   float* __restrict__ value_out, const float* __restrict__ aux_dev,
                                                                   float* __restrict__ aux_out) {
    const int w = blockIdx.x;
    const int board = board_of[w];
    if (threadIdx.x == 0) value_out[board] = value_dev[w];
    if (aux_dev != nullptr && threadIdx.x < 4) aux_out[board * 4 + threadIdx.x] = aux_dev[w * 4 + threadIdx.x];
    const float* src = probs + size_t(w) * nb_policy;
    float* dst = probs_out + size_t(board) * nb_policy;
    for (int i = threadIdx.x; i < nb_policy; i += 256) dst[i] = src[i];
    if (logits != nullptr) {
        src = logits + size_t(w) * nb_policy;
        dst = logits_out + size_t(board) * nb_policy;
        for (int i = threadIdx.x; i < nb_policy; i += 256) dst[i] = src[i];
    }
}
void launch_scatter_rows_indexed(const float* probs, const float* logits, int nb_policy, const int* board_of, int n_slots, float* probs_out,
                                 float* logits_out, const float* value_dev, float* value_out, const float* aux_dev, float* aux_out, hipStream_t s) {
    hipLaunchKernelGGL(scatter_rows_indexed_kernel, dim3(n_slots), dim3(256), 0, s, probs, logits, nb_policy, board_of, probs_out, logits_out,
                       value_dev, value_out, aux_dev, aux_out);
}

// float planes of a group out of the batch's planes: dst slot w = src board board_of[w] (row = C * 64 floats)
__global__ __launch_bounds__(256) void gather_planes_indexed_kernel(const float* __restrict__ src, const int* __restrict__ board_of, int row,
                                                                    float* __restrict__ dst) {
    const float* in = src + size_t(board_of[blockIdx.x]) * row;
    float* out = dst + size_t(blockIdx.x) * row;
    for (int i = threadIdx.x; i < row; i += 256) out[i] = in[i];
}
void launch_gather_planes_indexed(const float* src, const int* board_of, int n_slots, int row, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(gather_planes_indexed_kernel, dim3(n_slots), dim3(256), 0, s, src, board_of, row, dst);
}

void launch_softmax(const float* logits, float* probs, int batch, int n, hipStream_t s) {
    hipLaunchKernelGGL(softmax_kernel, dim3(batch), dim3(256), 0, s, logits, probs, n);
}

// ================================================================================================================
// NCHW float planes -> NHWC activation (channel padded with zeros).  LDS transpose, coalesced on both sides.
// ================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void planes_to_act_kernel(const float* __restrict__ planes, T* __restrict__ act, int C, int cpad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sp = reinterpret_cast<float*>(smem);   // [C][65]
    const float* pb = planes + size_t(blockIdx.x) * C * kSquares;
    for (int i = threadIdx.x; i < C * kSquares; i += 256) sp[(i >> 6) * 65 + (i & 63)] = pb[i];
    __syncthreads();
    T* ab = act + size_t(blockIdx.x) * kSquares * cpad;
    for (int i = threadIdx.x; i < kSquares * cpad; i += 256) {
        const int sq = i / cpad, c = i - sq * cpad;
        ab[i] = T(c < C ? sp[c * 65 + sq] : 0.f);
    }
}

template <typename T> void launch_planes_to_act(const float* planes, T* act, int batch, int C, int cpad, hipStream_t s) {
    hipLaunchKernelGGL((planes_to_act_kernel<T>), dim3(batch), dim3(256), size_t(C) * 65 * sizeof(float), s, planes, act, C, cpad);
}
template void launch_planes_to_act<half_t>(const float*, half_t*, int, int, int, hipStream_t);
template void launch_planes_to_act<float>(const float*, float*, int, int, int, hipStream_t);

}  // namespace cra

// ================================================================================================================
// Fused bottleneck block: expand (MFMA) -> depthwise (VALU, via LDS) -> project (MFMA, register accumulator) -> +x
// ================================================================================================================
namespace cra {

template <typename T, int KS, int NW> struct BlockGeomK {
    static constexpr int C = 256;                       // residual-stream width the kernel is specialised for
    static constexpr int CK = 16 * NW;                  // C_op channels per chunk: one 16-channel MFMA tile per wave
    static constexpr int NTHR = 64 * NW;
    static constexpr int PAD = 16 / int(sizeof(T));
    static constexpr int XROW = C + PAD;
    static constexpr int TROW = CK + PAD;
    static constexpr int WDW = KS * KS * CK + 2 * CK;   // floats: depthwise taps [KS*KS][CK], then b1[CK], b2[CK] of the chunk
    static constexpr size_t lds_bytes = (size_t(64) * XROW + 2 * size_t(64) * TROW) * sizeof(T) + size_t(WDW) * sizeof(float);
};

// Software pipeline per chunk (4 waves, one board):
//   E  expand MFMAs (w1 fragments prefetched into registers during the previous P phase; x tile from LDS)
//      -> epilogue writes the chunk's 64 x 64 tile t1 (+BN1 bias, ReLU) and parks the prefetched depthwise taps/biases in LDS
//   -- barrier --   (w3 fragments of this chunk are requested here, they land while D runs)
//   D  depthwise k x k on the VALU from t1 (taps in registers for 3x3), +BN2 bias, ReLU -> t2
//   -- barrier --   (w1 fragments + depthwise taps + biases of the NEXT chunk are requested here, they land while P runs)
//   P  project MFMAs into the 64(cout) x 64(square) register accumulator of each wave
template <typename T, int KS, int NW>
__global__ __launch_bounds__(64 * NW) void block_kernel(const BlockArgs a) {
    using frag = typename VT<T>::frag;
    using G = BlockGeomK<T, KS, NW>;
    constexpr int C = G::C, CK = G::CK, XROW = G::XROW, TROW = G::TROW, NT = KS * KS, NTHR = G::NTHR;
    constexpr int NW4 = (NT * CK + 2 * CK) / 4;          // float4s of per-chunk depthwise parameters
    constexpr int W4_PER_THREAD = (NW4 + NTHR - 1) / NTHR;
    constexpr int NJ = C / 16 / NW;                      // cout tiles per wave in the project phase
    constexpr int NCG = CK / 8;                          // 8-channel groups per chunk (depthwise thread mapping)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs = reinterpret_cast<T*>(smem);          // [64][XROW]  block input (also the residual)
    T* t1 = xs + 64 * XROW;                      // [64][TROW]  expand output of the current chunk
    T* t2 = t1 + 64 * TROW;                      // [64][TROW]  depthwise output of the current chunk
    float* wl = reinterpret_cast<float*>(t2 + 64 * TROW);   // [NT][CK] taps, b1[CK], b2[CK]

    const int b = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int nchunk = a.cop_pad / CK;
    const int nslab3 = a.cop_pad >> 5;
    const frag* w1base = reinterpret_cast<const frag*>(a.w1pk) + lane;
    const frag* w3base = reinterpret_cast<const frag*>(a.w3pk) + lane;

    // per-chunk depthwise parameter prefetch: element i of [taps | b1 | b2] (float4 granularity)
    auto dw_param_ptr = [&](int ch, int i4) -> const float* {
        const int e = i4 * 4;
        if (e < NT * CK) return a.wdw + size_t(e / CK) * a.cop_pad + ch * CK + (e % CK);
        if (e < NT * CK + CK) return a.b1 + ch * CK + (e - NT * CK);
        return a.b2 + ch * CK + (e - NT * CK - CK);
    };
    frag w1f[C / 32];
    f32x4 dwp[W4_PER_THREAD];
    auto prefetch_chunk = [&](int ch) {
        const frag* w1 = w1base + size_t(ch * NW + wave) * (C / 32) * 64;
#pragma unroll
        for (int s = 0; s < C / 32; ++s) w1f[s] = w1[s * 64];
#pragma unroll
        for (int k = 0; k < W4_PER_THREAD; ++k) {
            const int i4 = tid + k * NTHR;
            if (i4 < NW4) dwp[k] = *reinterpret_cast<const f32x4*>(dw_param_ptr(ch, i4));
        }
    };
    prefetch_chunk(0);

    const T* xb = reinterpret_cast<const T*>(a.x) + size_t(b) * 64 * C;
    {
        constexpr int vec_per_row = C * int(sizeof(T)) / 16;
        if (a.gate == nullptr) {
            for (int i = tid; i < 64 * vec_per_row; i += NTHR) {
                const int r = i / vec_per_row, v = i - r * vec_per_row;
                *reinterpret_cast<uint4*>(reinterpret_cast<char*>(xs + r * XROW) + v * 16) =
                    *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(xb + size_t(r) * C) + v * 16);
            }
        } else {   // x := x * gate[b][c]  (_ChannelAttentionModule.forward: x * y.expand_as(x), builder_util.py:114)
            constexpr int EPV = 16 / int(sizeof(T));     // elements per 16-byte vector
            const float* g = a.gate + size_t(b) * C;
            for (int i = tid; i < 64 * vec_per_row; i += NTHR) {
                const int r = i / vec_per_row, v = i - r * vec_per_row;
                float xv[EPV], gv[EPV];
                if constexpr (EPV == 8) { load8<T>(xb + size_t(r) * C + v * 8, xv); load8<float>(g + v * 8, gv); }
                else { load4<T>(xb + size_t(r) * C + v * 4, xv); load4<float>(g + v * 4, gv); }
#pragma unroll
                for (int j = 0; j < EPV; ++j) xv[j] *= gv[j];
                if constexpr (EPV == 8) store8<T>(xs + r * XROW + v * 8, xv);
                else store4<T>(xs + r * XROW + v * 4, xv);
            }
        }
    }
    __syncthreads();

    f32x4 accP[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) accP[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // depthwise thread mapping: 8 channels x 2 squares
    const int cg = tid % NCG, sqb = tid / NCG;

    for (int ch = 0; ch < nchunk; ++ch) {
        // ---------------- E: expand, 16 channels x 64 squares per wave, K = C ----------------
        f32x4 accE[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) accE[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < C / 32; ++s) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const frag bf = *reinterpret_cast<const frag*>(xs + (t * 16 + l15) * XROW + s * 32 + lg * 8);
                mma_k32(w1f[s], bf, accE[t]);
            }
        }
        // park this chunk's depthwise parameters in LDS (wl was last read in the previous chunk's D phase, two barriers ago)
#pragma unroll
        for (int k = 0; k < W4_PER_THREAD; ++k) {
            const int i4 = tid + k * NTHR;
            if (i4 < NW4) *reinterpret_cast<f32x4*>(wl + i4 * 4) = dwp[k];
        }
        __syncthreads();   // wl visible (b1 is read from it right below); also orders t1 writes after the previous D reads
        {
            const int cl = wave * 16 + lg * 4;           // channel inside the chunk
            float bs[4];
            load4<float>(wl + NT * CK + cl, bs);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(accE[t][r] + bs[r], 0.f);
                store4<T>(t1 + (t * 16 + l15) * TROW + cl, v);
            }
        }
        // request this chunk's project fragments now; they land while the depthwise phase runs
        frag w3f[CK / 32][NJ];
#pragma unroll
        for (int s2 = 0; s2 < CK / 32; ++s2)
#pragma unroll
            for (int j = 0; j < NJ; ++j) w3f[s2][j] = w3base[(size_t(wave * NJ + j) * nslab3 + ch * (CK / 32) + s2) * 64];
        __syncthreads();
        // ---------------- D: depthwise k x k + BN + ReLU (fp32 accumulate) ----------------
        {
            float bias2[8];
            load8<float>(wl + NT * CK + CK + cg * 8, bias2);
            if constexpr (KS == 3) {
                float wr[9][8];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) load8<float>(wl + tap * CK + cg * 8, wr[tap]);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int sq = sqb + 32 * jj;
                    const int py = sq >> 3, px = sq & 7;
                    float acc[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = bias2[j];
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        const int ny = py + tap / 3 - 1, nx = px + tap % 3 - 1;
                        if ((unsigned(ny) < 8u) && (unsigned(nx) < 8u)) {
                            float xv[8];
                            load8<T>(t1 + (ny * 8 + nx) * TROW + cg * 8, xv);
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc[j] = fmaf(wr[tap][j], xv[j], acc[j]);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaxf(acc[j], 0.f);
                    store8<T>(t2 + sq * TROW + cg * 8, acc);
                }
            } else {
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int sq = sqb + 32 * jj;
                    const int py = sq >> 3, px = sq & 7;
                    float acc[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = bias2[j];
#pragma unroll
                    for (int tap = 0; tap < NT; ++tap) {
                        const int ny = py + tap / KS - KS / 2, nx = px + tap % KS - KS / 2;
                        if ((unsigned(ny) < 8u) && (unsigned(nx) < 8u)) {
                            float xv[8], wv[8];
                            load8<T>(t1 + (ny * 8 + nx) * TROW + cg * 8, xv);
                            load8<float>(wl + tap * CK + cg * 8, wv);
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc[j] = fmaf(wv[j], xv[j], acc[j]);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaxf(acc[j], 0.f);
                    store8<T>(t2 + sq * TROW + cg * 8, acc);
                }
            }
        }
        __syncthreads();
        // request the next chunk's expand fragments / depthwise parameters; they land while the project MFMAs run
        if (ch + 1 < nchunk) prefetch_chunk(ch + 1);
        // ---------------- P: project, 64 couts x 64 squares per wave, K = CK (accumulates over chunks) ----------------
#pragma unroll
        for (int s2 = 0; s2 < CK / 32; ++s2) {
            frag bf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) bf[t] = *reinterpret_cast<const frag*>(t2 + (t * 16 + l15) * TROW + s2 * 32 + lg * 8);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) mma_k32(w3f[s2][j], bf[t], accP[j][t]);
        }
    }

    // ---------------- epilogue: + BN3 bias + residual (the SE-scaled input tile) ----------------
    T* yb = reinterpret_cast<T*>(a.y) + size_t(b) * 64 * C;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int co0 = (wave * NJ + j) * 16 + lg * 4;
        float bs[4];
        load4<float>(a.b3 + co0, bs);
        float pool[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sq = t * 16 + l15;
            float rv[4], v[4];
            load4<T>(xs + sq * XROW + co0, rv);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = accP[j][t][r] + bs[r] + rv[r];
                pool[r] += to_f(T(v[r]));               // pool what the next block will read
            }
            store4<T>(yb + size_t(sq) * C + co0, v);
        }
        if (a.pool_out) {                               // squeeze (AdaptiveAvgPool2d) of the block output, fused here
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) pool[r] += __shfl_xor(pool[r], off, 64);
            if (l15 == 0) store4<float>(a.pool_out + size_t(b) * C + co0, pool);
        }
    }
}

// ================================================================================================================
// 3x3 variant: the depthwise convolution runs directly on the expand accumulators with DPP lane shifts.
//
// An MFMA 16x16 D tile holds, in lane (l15, lg), square = t*16 + l15 of channels lg*4..lg*4+3.  A board row is 8 squares,
// so inside one 16-lane DPP row the horizontal neighbours are lanes l15 -/+ 1 (row_shr:1 / row_shl:1) and the vertical
// neighbours are lane (l15 + 8) % 16 (row_ror:8) of the same tile (l15 < 8: the row above lives in tile t-1) -- every one
// of the 9 taps of a channel is reachable without leaving the 16-lane row that owns the channel.  Edge masks (file a / h,
// rank 1 / 8) are folded into the per-lane tap weights.  Result: no LDS round trip for the expand output, no f16<->f32
// conversions, no bounds branches; LDS only carries the x tile (B operand of expand) and the depthwise output t2
// (B operand of project).
// ================================================================================================================

template <typename T, int NW> struct BlockGeomD {
    static constexpr int C = 256;
    static constexpr int CK = 16 * NW;
    static constexpr int NTHR = 64 * NW;
    static constexpr int PAD = 32 / int(sizeof(T));     // 32-byte row pad: rows step 8 banks -> conflict-free 16-row fragment reads
    static constexpr int XROW = C + PAD;
    static constexpr int TROW = CK + PAD;
    static constexpr size_t lds_bytes = (size_t(64) * XROW + size_t(64) * TROW) * sizeof(T);
};

template <typename T, int NW>
__global__ __launch_bounds__(64 * NW) void block_kernel_dpp(const BlockArgs a) {
    using frag = typename VT<T>::frag;
    using G = BlockGeomD<T, NW>;
    constexpr int C = G::C, CK = G::CK, XROW = G::XROW, TROW = G::TROW, NTHR = G::NTHR;
    constexpr int NJ = C / 16 / NW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs = reinterpret_cast<T*>(smem);          // [64][XROW]
    T* t2 = xs + 64 * XROW;                      // [64][TROW]  depthwise output of the current chunk

    const int b = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int nchunk = a.cop_pad / CK;
    const int nslab3 = a.cop_pad >> 5;
    const frag* w1base = reinterpret_cast<const frag*>(a.w1pk) + lane;
    const frag* w3base = reinterpret_cast<const frag*>(a.w3pk) + lane;
    const bool hi = l15 >= 8;                                  // second board row of the tile
    const float mL = (l15 & 7) != 0 ? 1.f : 0.f;               // a left / right neighbour exists on the board
    const float mR = (l15 & 7) != 7 ? 1.f : 0.f;

    frag w1f[C / 32];
    f32x4 dwr[4][3];                                           // [channel r][float4 k] = 12 floats of dwpk per channel
    auto prefetch_chunk = [&](int ch) {
        const frag* w1 = w1base + size_t(ch * NW + wave) * (C / 32) * 64;
#pragma unroll
        for (int s = 0; s < C / 32; ++s) w1f[s] = w1[s * 64];
        const f32x4* dp = reinterpret_cast<const f32x4*>(a.dwpk + size_t(ch * CK + wave * 16 + lg * 4) * 12);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) dwr[r][k] = dp[r * 3 + k];
    };
    prefetch_chunk(0);

    const T* xb = reinterpret_cast<const T*>(a.x) + size_t(b) * 64 * C;
    {
        constexpr int vec_per_row = C * int(sizeof(T)) / 16;
        if (a.gate == nullptr) {
            for (int i = tid; i < 64 * vec_per_row; i += NTHR) {
                const int r = i / vec_per_row, v = i - r * vec_per_row;
                *reinterpret_cast<uint4*>(reinterpret_cast<char*>(xs + r * XROW) + v * 16) =
                    *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(xb + size_t(r) * C) + v * 16);
            }
        } else {
            constexpr int EPV = 16 / int(sizeof(T));
            const float* g = a.gate + size_t(b) * C;
            for (int i = tid; i < 64 * vec_per_row; i += NTHR) {
                const int r = i / vec_per_row, v = i - r * vec_per_row;
                float xv[EPV], gv[EPV];
                if constexpr (EPV == 8) { load8<T>(xb + size_t(r) * C + v * 8, xv); load8<float>(g + v * 8, gv); }
                else { load4<T>(xb + size_t(r) * C + v * 4, xv); load4<float>(g + v * 4, gv); }
#pragma unroll
                for (int j = 0; j < EPV; ++j) xv[j] *= gv[j];
                if constexpr (EPV == 8) store8<T>(xs + r * XROW + v * 8, xv);
                else store4<T>(xs + r * XROW + v * 4, xv);
            }
        }
    }
    __syncthreads();

    f32x4 accP[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) accP[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < nchunk; ++ch) {
        // ---------------- E: expand, 16 channels x 64 squares per wave, K = C ----------------
        f32x4 accE[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) accE[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < C / 32; ++s) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const frag bf = *reinterpret_cast<const frag*>(xs + (t * 16 + l15) * XROW + s * 32 + lg * 8);
                mma_k32(w1f[s], bf, accE[t]);
            }
        }
        // request this chunk's project fragments; they land while the depthwise runs
        frag w3f[CK / 32][NJ];
#pragma unroll
        for (int s2 = 0; s2 < CK / 32; ++s2)
#pragma unroll
            for (int j = 0; j < NJ; ++j) w3f[s2][j] = w3base[(size_t(wave * NJ + j) * nslab3 + ch * (CK / 32) + s2) * 64];

        // ---------------- D: BN1 + ReLU, depthwise 3x3 on the accumulators, BN2 + ReLU ----------------
        float outv[4][4];                                       // [tile][channel r]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float b1 = dwr[r][2][1], b2 = dwr[r][2][2];
            float w[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = dwr[r][k >> 2][k & 3];
            // taps: k = (dy+1)*3 + (dx+1); fold the file-edge masks into the dx = -1 / +1 columns
            w[0] *= mL; w[3] *= mL; w[6] *= mL;
            w[2] *= mR; w[5] *= mR; w[8] *= mR;
            float e[4], rot[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                e[t] = fmaxf(accE[t][r] + b1, 0.f);
                rot[t] = dpp_mov<DPP_ROW_ROR8>(e[t]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                // square above (dy = -1) / below (dy = +1): same tile for one half of the lanes, neighbouring tile for the other
                const float up = hi ? rot[t] : (t > 0 ? rot[t > 0 ? t - 1 : 0] : 0.f);
                const float dn = hi ? (t < 3 ? rot[t < 3 ? t + 1 : 3] : 0.f) : rot[t];
                float acc = b2;
                acc = fmaf(w[0], dpp_mov<DPP_ROW_SHR1>(up), acc);
                acc = fmaf(w[1], up, acc);
                acc = fmaf(w[2], dpp_mov<DPP_ROW_SHL1>(up), acc);
                acc = fmaf(w[3], dpp_mov<DPP_ROW_SHR1>(e[t]), acc);
                acc = fmaf(w[4], e[t], acc);
                acc = fmaf(w[5], dpp_mov<DPP_ROW_SHL1>(e[t]), acc);
                acc = fmaf(w[6], dpp_mov<DPP_ROW_SHR1>(dn), acc);
                acc = fmaf(w[7], dn, acc);
                acc = fmaf(w[8], dpp_mov<DPP_ROW_SHL1>(dn), acc);
                outv[t][r] = fmaxf(acc, 0.f);
            }
        }
        {
            const int cl = wave * 16 + lg * 4;
#pragma unroll
            for (int t = 0; t < 4; ++t) store4<T>(t2 + (t * 16 + l15) * TROW + cl, outv[t]);
        }
        __syncthreads();
        if (ch + 1 < nchunk) prefetch_chunk(ch + 1);
        // ---------------- P: project, accumulates over chunks ----------------
#pragma unroll
        for (int s2 = 0; s2 < CK / 32; ++s2) {
            frag bf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) bf[t] = *reinterpret_cast<const frag*>(t2 + (t * 16 + l15) * TROW + s2 * 32 + lg * 8);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) mma_k32(w3f[s2][j], bf[t], accP[j][t]);
        }
        __syncthreads();   // t2 is rewritten by the next chunk's depthwise
    }

    T* yb = reinterpret_cast<T*>(a.y) + size_t(b) * 64 * C;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int co0 = (wave * NJ + j) * 16 + lg * 4;
        float bs[4];
        load4<float>(a.b3 + co0, bs);
        float pool[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sq = t * 16 + l15;
            float rv[4], v[4];
            load4<T>(xs + sq * XROW + co0, rv);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = accP[j][t][r] + bs[r] + rv[r];
                pool[r] += to_f(T(v[r]));
            }
            store4<T>(yb + size_t(sq) * C + co0, v);
        }
        if (a.pool_out) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) pool[r] += __shfl_xor(pool[r], off, 64);
            if (l15 == 0) store4<float>(a.pool_out + size_t(b) * C + co0, pool);
        }
    }
}

template <typename T> struct BlockWaves;
template <> struct BlockWaves<half_t> { static constexpr int NW = 8; };   // 512 threads: two waves per SIMD hide LDS / MFMA latencies
template <> struct BlockWaves<float> { static constexpr int NW = 4; };    // f32 fragments are twice as wide: stay at one wave per SIMD

template <typename T> void init_block_kernel_attributes() {
    constexpr int NW = BlockWaves<T>::NW;
    constexpr int lds3 = int(BlockGeomK<T, 3, NW>::lds_bytes), lds5 = int(BlockGeomK<T, 5, NW>::lds_bytes);
    auto k3 = &block_kernel<T, 3, NW>;
    auto k5 = &block_kernel<T, 5, NW>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k3), hipFuncAttributeMaxDynamicSharedMemorySize, lds3);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k5), hipFuncAttributeMaxDynamicSharedMemorySize, lds5);
    auto kd = &block_kernel_dpp<T, NW>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kd), hipFuncAttributeMaxDynamicSharedMemorySize, int(BlockGeomD<T, NW>::lds_bytes));
}
template void init_block_kernel_attributes<half_t>();
template void init_block_kernel_attributes<float>();

template <typename T> int block_chunk_channels() { return BlockGeomK<T, 3, BlockWaves<T>::NW>::CK; }
template int block_chunk_channels<half_t>();
template int block_chunk_channels<float>();

template <typename T> void launch_block(const BlockArgs& a, hipStream_t s) {
    constexpr int NW = BlockWaves<T>::NW;
    constexpr size_t lds3 = BlockGeomK<T, 3, NW>::lds_bytes, lds5 = BlockGeomK<T, 5, NW>::lds_bytes;
    auto k3 = &block_kernel<T, 3, NW>;
    auto k5 = &block_kernel<T, 5, NW>;
    auto kd = &block_kernel_dpp<T, NW>;
    constexpr size_t ldsd = BlockGeomD<T, NW>::lds_bytes;
    if (a.ks == 3 && a.dwpk) hipLaunchKernelGGL(kd, dim3(a.batch), dim3(64 * NW), ldsd, s, a);
    else if (a.ks == 3) hipLaunchKernelGGL(k3, dim3(a.batch), dim3(64 * NW), lds3, s, a);
    else hipLaunchKernelGGL(k5, dim3(a.batch), dim3(64 * NW), lds5, s, a);
}
template void launch_block<half_t>(const BlockArgs&, hipStream_t);
template void launch_block<float>(const BlockArgs&, hipStream_t);

}  // namespace cra
