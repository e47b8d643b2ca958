// Device helpers of the float16x3 conv GEMMs that more than one translation unit needs (x3.hip: conv_gemm_x3_kernel, the policy chain
// conv3x3_x3_chain_kernel; x3_heads.cpp: the chain with the value head on its idle waves): the staging geometry, the epilogue of the conv
// GEMMs with the board's softmax, and the pieces of the chain -- its two staging buffers, the weight window, a staged pass, the staging
// registers.  Needs x3_device.h (the split).  Internal linkage or always inlined: each translation unit has its own copy.
#pragma once
#include "kernels.h"
#include "device_utils.h"
#include "x3_device.h"

namespace cra {

namespace {
constexpr int X3_KC = 128;                 // input channels staged per pass of the conv GEMM
constexpr int X3_ROWP = X3_KC + 8;         // halves per LDS row (+16 B: the 16 rows of a fragment read land in 16 bank groups)
}  // namespace

// The epilogue of the conv GEMMs: conv_gemm_kernel<float>'s, word for word (bias, ReLU before / after the shortcut, the four output layouts,
// the fused row softmax); acc_scale: the accumulators carry the weights' power-of-two scale (Precision float16p8)
template <int MT, int NW>
__device__ __forceinline__ void conv_x3_finish(const ConvArgs& a, f32x4 (&acc)[MT][4], const bool (&active)[MT], char* smem, int b, int co_tile0, float acc_scale) {
    constexpr int NTHR = 64 * NW;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int l15 = lane & 15, lg = lane >> 4;
    if (a.softmax_out) __syncthreads();                      // the board's logits gather in the staging tiles: every wave is done reading them
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (!active[m]) continue;
        const int co0 = (co_tile0 + m) * 16 + lg * 4;
        float bs[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bs[r] = a.bias[co0 + r];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sq = t * 16 + l15;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaf(acc[m][t][r], acc_scale, bs[r]);
            if (a.relu == 2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            if (a.resid) {
                float rv[4];
                load4<float>(reinterpret_cast<const float*>(a.resid) + (size_t(b) * kSquares + sq) * a.cout_ld + co0, rv);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += rv[r];
            }
            if (a.relu == 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            if (a.out_policy_f32) {
                float* o = reinterpret_cast<float*>(a.out) + size_t(b) * a.cout_real * kSquares;
                float* lds_logits = reinterpret_cast<float*>(smem);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co0 + r < a.cout_real) {
                        if (a.out) o[(co0 + r) * kSquares + sq] = v[r];
                        if (a.softmax_out) lds_logits[(co0 + r) * kSquares + sq] = v[r];
                    }
            } else if (a.out_rows_f32) {
                const int row = b * kSquares + sq;
                if (row < a.rows_valid) {
                    float* o = reinterpret_cast<float*>(a.out) + size_t(row) * a.cout_real;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (co0 + r < a.cout_real) o[co0 + r] = v[r];
                }
            } else if (a.out_flat) {
                float* o = reinterpret_cast<float*>(a.out) + size_t(b) * a.flat_pitch;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co0 + r < a.cout_real) o[(co0 + r) * kSquares + sq] = v[r];
            } else {
                store4<float>(reinterpret_cast<float*>(a.out) + (size_t(b) * kSquares + sq) * a.cout_ld + co0, v);
            }
        }
    }
    if (a.softmax_out) {
        // row softmax of the board's logits (softmax_kernel, kernels.hip; apply_softmax(), neuralnetapi.cpp:241-260): exp(x - (max + log(sum)))
        __syncthreads();
        const float* in = reinterpret_cast<const float*>(smem);
        float* red = reinterpret_cast<float*>(smem) + 8192;  // behind the logits (at most 8192 of them: 32 KiB of the 35 KiB)
        const int n = a.cout_real * kSquares;
        float* out = a.softmax_out + size_t(b) * n;
        float m = -INFINITY;
        for (int i = tid; i < n; i += NTHR) m = fmaxf(m, in[i]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        if (lane == 0) red[wave] = m;
        __syncthreads();
        m = red[0];
#pragma unroll
        for (int i = 1; i < NW; ++i) m = fmaxf(m, red[i]);
        float sum = 0.f;
        for (int i = tid; i < n; i += NTHR) sum += expf(in[i] - m);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        __syncthreads();
        if (lane == 0) red[wave] = sum;
        __syncthreads();
        sum = red[0];
#pragma unroll
        for (int i = 1; i < NW; ++i) sum += red[i];
        const float c = m + logf(sum);
        for (int i = tid; i < n; i += NTHR) out[i] = expf(in[i] - c);
    }
}

// ---- the policy chain's pieces (x3.hip: conv3x3_x3_chain_kernel) ----
namespace {
struct ConvX3 {
    static constexpr int KC = X3_KC, ROWP = X3_ROWP, NS = KC / 32, NSTEP = 9 * NS, D = 3;
    static constexpr size_t buf_bytes = size_t(2) * 65 * ROWP * sizeof(half_t);          // hi tile + lo tile, 65 rows (row 64: zeros)
    static constexpr size_t lds_bytes = 2 * buf_bytes;                                     // 70.7 KB
    static __device__ __forceinline__ half_t* xh_of(char* smem, int buf) { return reinterpret_cast<half_t*>(smem + buf * buf_bytes); }
    static __device__ __forceinline__ half_t* xl_of(char* smem, int buf) { return xh_of(smem, buf) + 65 * ROWP; }
};
template <int MT> struct ConvX3Window { half8 wh[ConvX3::D][MT], wl[ConvX3::D][MT]; };
template <int MT>
__device__ __forceinline__ void conv_x3_wload(ConvX3Window<MT>& W, const half8* const (&wph)[MT], const half8* const (&wpl)[MT], int kc0, int nslab_ci, int st) {
    const size_t wo = size_t((st / ConvX3::NS) * nslab_ci + (kc0 >> 5) + st % ConvX3::NS) * 64;      // step st = tap st / NS, k-slab st % NS of this pass
#pragma unroll
    for (int m = 0; m < MT; ++m) { W.wh[st % ConvX3::D][m] = wph[m][wo]; W.wl[st % ConvX3::D][m] = wpl[m][wo]; }
}
template <int MT>
__device__ __forceinline__ void conv_x3_prime(ConvX3Window<MT>& W, const half8* const (&wph)[MT], const half8* const (&wpl)[MT], int kc0, int nslab_ci) {
#pragma unroll
    for (int st = 0; st < ConvX3::D; ++st) conv_x3_wload<MT>(W, wph, wpl, kc0, nslab_ci, st);
}
// the 9 taps x 4 k-slabs of one staged pass: conv_gemm_x3_body's static schedule (NS = 4), window primed by the caller
template <int MT>
__device__ __forceinline__ void conv_x3_pass(ConvX3Window<MT>& W, const half_t* xh, const half_t* xl, const half8* const (&wph)[MT],
                                             const half8* const (&wpl)[MT], int kc0, int nslab_ci, int l15, int lg, f32x4 (&acc)[MT][4]) {
    constexpr int ROWP = ConvX3::ROWP, NS = ConvX3::NS, NSTEP = ConvX3::NSTEP, D = ConvX3::D;
    half8 bh[2][4], bl[2][4];
    auto read_frag = [&](int st) {
        const int tap = st / NS, sl = st % NS, dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sq = t * 16 + l15;
            const int ny = (sq >> 3) + dy, nx = (sq & 7) + dx;
            const bool ok = (unsigned(ny) < 8u) && (unsigned(nx) < 8u);
            const int off = (ok ? ny * 8 + nx : 64) * ROWP + lg * 8 + sl * 32;
            bh[st & 1][t] = *reinterpret_cast<const half8*>(xh + off);
            bl[st & 1][t] = *reinterpret_cast<const half8*>(xl + off);
        }
    };
    read_frag(0);
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
        if (st + 1 < NSTEP) read_frag(st + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(W.wl[st % D][m], bh[st & 1][t], acc[m][t], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(W.wh[st % D][m], bl[st & 1][t], acc[m][t], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(W.wh[st % D][m], bh[st & 1][t], acc[m][t], 0, 0, 0);
        if (st + D < NSTEP) conv_x3_wload<MT>(W, wph, wpl, kc0, nslab_ci, st + D);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// stages one board's input channels [kc0, kc0 + 128) as split tiles: `request` into registers, `split_store` from them (512 threads)
struct ConvX3Stage {
    static constexpr int NV = kSquares * (ConvX3::KC / 8) / 512;
    float pre[NV][8];
    __device__ __forceinline__ void request(const float* xb, int cin, int kc0, int tid) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = tid + j * 512, r = i / (ConvX3::KC / 8), v = i - r * (ConvX3::KC / 8);
            load8<float>(xb + size_t(r) * cin + kc0 + v * 8, pre[j]);
        }
    }
    __device__ __forceinline__ void split_store(half_t* xh, half_t* xl, int tid) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = tid + j * 512, r = i / (ConvX3::KC / 8), v = i - r * (ConvX3::KC / 8);
            half8 h, l;
            split8(pre[j], h, l);
            *reinterpret_cast<half8*>(xh + r * ConvX3::ROWP + v * 8) = h;
            *reinterpret_cast<half8*>(xl + r * ConvX3::ROWP + v * 8) = l;
        }
    }
};
}  // namespace

}  // namespace cra
