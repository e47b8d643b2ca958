// Precision float16x3: the policy head and the value head of a policy-map net in ONE launch, for nets made for more than 64 boards.
//
// conv3x3_x3_heads_kernel is conv3x3_x3_chain_kernel (x3.hip) step for step -- the staging, conv_x3_pass<2> on both passes, the conv 1
// epilogue split into the two buffers, conv_x3_pass<1>, conv_x3_finish<1, 8>, every barrier in the same place -- so the logits and the
// probabilities are the chain's bits by construction.  The second conv (at most six cout tiles here) runs one tile per wave: waves 6 and 7
// have none and wait at the next barrier for its 72 steps.  They run the value head instead.
//
// The value role is value_head_body<float, false, true, 512>'s arithmetic (value_head_body.h), term for term, on other threads:
//   * the f32 board is stored a second time, unsplit, from the staging registers (ConvX3Stage::pre) into a [64][256 + 4] tile behind the
//     chain's buffers: both heads read the board from HBM once.  The 8 KB of folded conv 1x1 weights go to LDS with the first pass.
//   * conv 1x1 + BN + ReLU after the barrier that ends conv 1: wave 6 value channels 0-3, wave 7 channels 4-7, lane = square, the body's
//     order over c (four fmaf per f32x4, channels 0 ... 255).
//   * FC1: group kq of the body (cv = 8, 512 threads) is value channel kq, so each wave needs only what it produced itself: no exchange.
//     Lane = four consecutive outputs, the inputs i = 0 ... 63 of a group in order, the body's v_fmac_f32 quadruple.  32 weight rows
//     (128 registers) in flight, refilled behind their products; the first 32 are requested BEFORE the conv 1x1.
//   * the tail (sum of the eight partial sums in the body's order, bias, ReLU, FC2, block_sum<512>, tanh) on all 512 threads behind a
//     barrier every wave reaches, in front of the policy epilogue.
// No flags, no spin waits: only workgroup barriers that all eight waves reach.
//
// LDS: 70,720 B chain tiles + 66,560 B board + 8 KB conv weights + 2 KB s_flat + 8 KB s_part + 32 B = 155,744 B of 160 KB; the chain is one
// workgroup per CU already (512 threads, 170 registers).
#include "x3_heads.h"
#include "device_utils.h"
#include "value_head_body.h"
#include "x3_device.h"
#include "x3_conv_device.h"

#include <stdexcept>

namespace cra {

namespace {
struct HeadsX3 {
    static constexpr int C = 256, CV = 8, FC = 256, XP = C + 4;        // XP: floats per row of the value head's board tile (rows step 4 banks)
    static constexpr size_t xs_off = ConvX3::lds_bytes;                                     // [64][XP] the board, f32
    static constexpr size_t ws_off = xs_off + size_t(kSquares) * XP * sizeof(float);        // [CV][C] folded conv 1x1 weights
    static constexpr size_t flat_off = ws_off + size_t(CV) * C * sizeof(float);             // [CV * 64] conv output, channel-major
    static constexpr size_t part_off = flat_off + size_t(CV) * kSquares * sizeof(float);    // [8 groups][FC] FC1 partial sums
    static constexpr size_t red_off = part_off + size_t(8) * FC * sizeof(float);            // [8]
    static constexpr size_t lds_bytes = red_off + 8 * sizeof(float);
};
static_assert(HeadsX3::xs_off % 16 == 0 && HeadsX3::lds_bytes <= 160 * 1024, "LDS budget");

// the staged floats of channels [kc0, kc0 + 128), unsplit, into the value head's board tile (ConvX3Stage's thread -> (row, 8 channels) map)
__device__ __forceinline__ void heads_x3_store_board(const ConvX3Stage& stage, float* xs, int kc0, int tid) {
#pragma unroll
    for (int j = 0; j < ConvX3Stage::NV; ++j) {
        const int i = tid + j * 512, r = i / (ConvX3::KC / 8), v = i - r * (ConvX3::KC / 8);
        float* p = xs + r * HeadsX3::XP + kc0 + v * 8;
        *reinterpret_cast<f32x4*>(p) = f32x4{stage.pre[j][0], stage.pre[j][1], stage.pre[j][2], stage.pre[j][3]};
        *reinterpret_cast<f32x4*>(p + 4) = f32x4{stage.pre[j][4], stage.pre[j][5], stage.pre[j][6], stage.pre[j][7]};
    }
}

// One of the two value waves (vw = 0: value channels / FC1 groups 0-3, vw = 1: 4-7): conv 1x1 + BN + ReLU into s_flat, FC1 partial sums of
// its four groups into s_part.  Reads only what this wave wrote of s_flat.
__device__ __forceinline__ void heads_x3_value_wave(const ValueHeadArgs& v, const float* xs, const float* ws, float* s_flat, float* s_part, int vw, int lane) {
    constexpr int C = HeadsX3::C, XP = HeadsX3::XP, FC = HeadsX3::FC;
    // FC1 rows of this wave: group kq, input i is row kq * 64 + i of w1t -- the wave's four groups are 256 consecutive rows, taken 32 at a time
    const float* wt = v.w1t + size_t(vw) * 256 * FC + 4 * lane;
    f32x4 w[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) w[j] = *reinterpret_cast<const f32x4*>(wt + size_t(j) * FC);      // (depend on nothing: in flight during the conv)
    __builtin_amdgcn_sched_barrier(0);                       // (the scheduler otherwise sinks the requests to their first use: a window of 8 - 12)
    {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const float* xr = xs + lane * XP;
        const float* wr = ws + vw * 4 * C;
#pragma unroll 2
        for (int c = 0; c < C; c += 4) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k * C + c);
                acc[k] = fmaf(wv[0], xv[0], acc[k]);
                acc[k] = fmaf(wv[1], xv[1], acc[k]);
                acc[k] = fmaf(wv[2], xv[2], acc[k]);
                acc[k] = fmaf(wv[3], xv[3], acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s_flat[(vw * 4 + k) * kSquares + lane] = fmaxf(acc[k] + v.bconv[vw * 4 + k], 0.f);
    }
    // the other lanes' conv outputs are this wave's own LDS writes: in order with its reads, no workgroup barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float* fl = s_flat + vw * 256;
    f32x4 h = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int bt = 0; bt < 8; ++bt) {                         // 32 inputs: half of group vw * 4 + bt / 2
        if ((bt & 1) == 0) h = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f32x4 f = *reinterpret_cast<const f32x4*>(fl + bt * 32 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * q + e;
                float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
                const float w0 = w[j][0], w1 = w[j][1], w2 = w[j][2], w3 = w[j][3], fe = f[e];
                // never v_pk_fma_f32 (build.py: NO_PACKED_FP32): the body's quadruple
                asm volatile("v_fmac_f32 %0, %4, %8\n\tv_fmac_f32 %1, %5, %8\n\tv_fmac_f32 %2, %6, %8\n\tv_fmac_f32 %3, %7, %8"
                             : "+v"(h0), "+v"(h1), "+v"(h2), "+v"(h3) : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(fe));
                h = f32x4{h0, h1, h2, h3};
                if (bt + 1 < 8) w[j] = *reinterpret_cast<const f32x4*>(wt + size_t((bt + 1) * 32 + j) * FC);
                __builtin_amdgcn_sched_barrier(0);           // the refill stays behind its product: 32 rows in flight
            }
        }
        if (bt & 1) *reinterpret_cast<f32x4*>(s_part + (vw * 4 + bt / 2) * FC + 4 * lane) = h;
    }
}
}  // namespace

__global__ __launch_bounds__(512) void conv3x3_x3_heads_kernel(const HeadsX3Args args) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ConvArgs& a = args.conv;
    const ValueHeadArgs& vh = args.vh;
    constexpr int KC = ConvX3::KC, ROWP = ConvX3::ROWP, NW = 8, C = 256;
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int l15 = lane & 15, lg = lane >> 4;
    const float* xb = reinterpret_cast<const float*>(a.x) + size_t(b) * kSquares * C;
    constexpr int nslab_ci = C >> 5, nslab = 9 * nslab_ci;
    float* xs = reinterpret_cast<float*>(smem + HeadsX3::xs_off);
    float* ws = reinterpret_cast<float*>(smem + HeadsX3::ws_off);
    float* s_flat = reinterpret_cast<float*>(smem + HeadsX3::flat_off);
    float* s_part = reinterpret_cast<float*>(smem + HeadsX3::part_off);
    float* s_red = reinterpret_cast<float*>(smem + HeadsX3::red_off);
    {   // ---- conv 1: this wave's two cout tiles of the 16
        const half8 *wph[2], *wpl[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            wph[m] = reinterpret_cast<const half8*>(a.pre_wpk) + size_t(wave * 2 + m) * nslab * 64 + lane;
            wpl[m] = reinterpret_cast<const half8*>(a.pre_wpk_lo) + size_t(wave * 2 + m) * nslab * 64 + lane;
        }
        f32x4 acc[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < 4 * ROWP; i += 512) {              // row 64 of all four tiles: what out-of-board taps read
            const int tile = i / ROWP, c = i - tile * ROWP;
            (tile & 1 ? ConvX3::xl_of(smem, tile >> 1) : ConvX3::xh_of(smem, tile >> 1))[64 * ROWP + c] = half_t(0.f);
        }
        const f32x4 wcv = *reinterpret_cast<const f32x4*>(vh.wconv + tid * 4);      // value head: the folded conv weights, 16 bytes per thread
        ConvX3Stage stage;
        stage.request(xb, C, 0, tid);
        stage.split_store(ConvX3::xh_of(smem, 0), ConvX3::xl_of(smem, 0), tid);
        heads_x3_store_board(stage, xs, 0, tid);
        *reinterpret_cast<f32x4*>(ws + tid * 4) = wcv;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            const int kc0 = pass * KC;
            ConvX3Window<2> W;
            conv_x3_prime<2>(W, wph, wpl, kc0, nslab_ci);
            __syncthreads();
            if (pass == 0) stage.request(xb, C, KC, tid);
            conv_x3_pass<2>(W, ConvX3::xh_of(smem, pass), ConvX3::xl_of(smem, pass), wph, wpl, kc0, nslab_ci, l15, lg, acc);
            if (pass == 0) {
                stage.split_store(ConvX3::xh_of(smem, 1), ConvX3::xl_of(smem, 1), tid);
                heads_x3_store_board(stage, xs, KC, tid);
            }
        }
        __syncthreads();                                         // every wave is through with the input tiles: they take conv 1's output
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int c0 = (wave * 2 + m) * 16 + lg * 4;         // 4 consecutive output channels of this lane
            const f32x4 bs = *reinterpret_cast<const f32x4*>(a.pre_bias + c0);
            half_t* xh = ConvX3::xh_of(smem, c0 >> 7);
            half_t* xl = ConvX3::xl_of(smem, c0 >> 7);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int sq = t * 16 + l15;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(fmaf(acc[m][t][r], 1.f, bs[r]), 0.f);      // (conv_x3_finish's form: fma by acc_scale = 1, ReLU)
                half4 h, l;
                split4(v, h, l);
                *reinterpret_cast<half4*>(xh + sq * ROWP + (c0 & 127)) = h;
                *reinterpret_cast<half4*>(xl + sq * ROWP + (c0 & 127)) = l;
            }
        }
    }
    // ---- conv 2: one cout tile per wave; the launcher takes at most six tiles, so waves 6 and 7 have none: the value head's two waves
    bool active[1] = {wave * 16 < a.cout_pad};
    const half8 *wph[1], *wpl[1];
    wph[0] = reinterpret_cast<const half8*>(a.wpk) + size_t(active[0] ? wave : 0) * nslab * 64 + lane;
    wpl[0] = reinterpret_cast<const half8*>(a.wpk_lo) + size_t(active[0] ? wave : 0) * nslab * 64 + lane;
    f32x4 acc2[1][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc2[0][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    ConvX3Window<1> W;
    if (active[0]) conv_x3_prime<1>(W, wph, wpl, 0, nslab_ci);
    float b1v = 0.f, w2v = 0.f;                                  // the value tail's two loads: back long before they are used
    if (tid < HeadsX3::FC) { b1v = vh.b1[tid]; w2v = vh.w2[tid]; }
    __syncthreads();                                             // conv 1's output tiles are written (and the value head's board and weights)
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    if (wave_u >= 6) {
        heads_x3_value_wave(vh, xs, ws, s_flat, s_part, wave_u - 6, lane);
    } else if (active[0]) {
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1) conv_x3_prime<1>(W, wph, wpl, KC, nslab_ci);
            conv_x3_pass<1>(W, ConvX3::xh_of(smem, pass), ConvX3::xl_of(smem, pass), wph, wpl, pass * KC, nslab_ci, l15, lg, acc2);
        }
    }
    __syncthreads();                                             // the eight groups' partial sums are in s_part
    {   // the value head's last stage, value_head_body's: thread = FC1 output
        float part = 0.f;
        if (tid < HeadsX3::FC) {
            constexpr int FC = HeadsX3::FC;
            const int t = tid;
            float ps = (s_part[t] + s_part[FC + t]) + (s_part[2 * FC + t] + s_part[3 * FC + t]);
            ps += (s_part[4 * FC + t] + s_part[5 * FC + t]) + (s_part[6 * FC + t] + s_part[7 * FC + t]);
            const float h = b1v + ps;
            part = fmaf(w2v, fmaxf(h, 0.f), part);
        }
        const float tot = block_sum<512>(part, s_red);
        if (tid == 0) vh.value[b] = tanhf(tot + vh.b2);
    }
    conv_x3_finish<1, NW>(a, acc2, active, smem, b, wave, 1.f);
}

bool heads_x3_fits(const ConvArgs& c, const ValueHeadArgs& v) {
    return c.pre_wpk && !c.p8 && c.ks == 3 && c.cin == HeadsX3::C && c.cout_pad <= 96 && !c.resid && !c.planes && !c.out_rows_f32 && c.out_policy_f32 &&
           !c.x_ld && c.dev == 0 && !v.wwdl && !v.dbg && v.variant == 0 && v.lds_pad < 0 && v.cv == HeadsX3::CV && v.fc == HeadsX3::FC && v.C == HeadsX3::C &&
           v.x == c.x && v.w1t && v.b1 && v.w2;
}
void init_x3_heads_kernel_attributes() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_x3_heads_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(HeadsX3::lds_bytes));
}
void launch_heads_x3(const HeadsX3Args& a, hipStream_t s) {
    if (!heads_x3_fits(a.conv, a.vh) || a.conv.batch != a.vh.batch)
        throw std::invalid_argument("conv3x3_x3_heads_kernel: the float16x3 policy chain with at most 96 padded couts and the plain value head (8 channels, 256 FC outputs) on the same boards");
    hipLaunchKernelGGL(conv3x3_x3_heads_kernel, dim3(1, a.conv.batch), dim3(512), HeadsX3::lds_bytes, s, a);
}

}  // namespace cra
