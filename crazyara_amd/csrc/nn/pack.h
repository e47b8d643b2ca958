// Host-side weight packing of the RISE nets: BN folding, the 8-bit number formats and every MFMA fragment / thread-order layout the
// kernels read (stream layouts in kernels.h).  Pure functions over the model file's tensors: no HIP runtime calls, no device memory --
// RiseNet::build uploads what they return.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "kernels.h"
#include "netfile.h"

namespace cra {

constexpr double kBnEps = 1e-5;   // torch.nn.BatchNorm2d default; the reference never overrides it

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// conv weight [cout][cin_g][k][k] + BN -> folded double weights / bias
struct Folded {
    std::vector<double> w;   // same layout as the input conv weight
    std::vector<double> b;   // [cout]
};
Folded fold_bn(const NetFile& nf, const std::string& conv, const std::string& bn);   // bn empty: the conv alone (zero bias)
// a bottleneck block's three folded layers: 1x1 expand (body.0/.1), depthwise (body.3/.4), 1x1 project (body.6/.7)
struct BlockFold { Folded expand, dw, project; };
BlockFold fold_block(const NetFile& nf, const std::string& prefix);

// A NextViT transformer block (NTB, next_vit_official_modules.py:267-335) folded for the layer kernels: every 1x1 / linear layer as a
// dense [cout][cin] Folded, BN folded in behind (patch_embed, projection, MHCA) or in front (norm1 into q / k / v, norm2 into mlp.conv1:
// merge_pre_bn, next_vit_official_modules.py:21-62), MHCA's grouped 3x3 as a block-diagonal dense 3x3.  Widths: D = E_MHSA channels,
// M = C - D (MHCA), H = the Mlp's hidden width.  Throws std::runtime_error naming the cause for what the layer path does not run:
// head_dim != 32, sr_ratio > 1 (e_mhsa.norm present), the "simple" variant (no projection / MHCA) and missing or mis-shaped tensors.
struct NtbFold {
    int C = 0, D = 0, M = 0, H = 0;
    Folded patch;       // [D][C]      conv1x1 + BN
    Folded qkv;         // [3D][D]     q, k, v rows (norm1 folded in), bias
    Folded proj;        // [D][D]      bias
    Folded projection;  // [M][D]      conv1x1 + BN
    Folded mhca;        // [M][M][3][3] block-diagonal grouped 3x3 + BN
    Folded mhca_proj;   // [M][M]      no bias
    Folded mlp1;        // [H][C]      norm2 folded in, bias
    Folded mlp2;        // [C][H]      bias
    double macs = 0;    // per position, the attention core included
};
NtbFold fold_ntb(const NetFile& nf, const std::string& prefix, int C);

uint8_t to_e4m3(double v);          // OCP e4m3fn, round to nearest even, clamps at +-448
uint8_t to_e5m2(float f);           // e5m2 ("bf8"), round to nearest even, saturating
double row_scale_pow2(double max_abs);

// MFMA A-fragment image of a dense layer (kernels.h); T = half_t or float
template <typename T> std::vector<T> pack_dense(const Folded& f, int cout, int cin, int ks, int cout_pad, int cin_pad);
// Precision float16x3: w = hi + lo, both f16, as two fragment images
struct SplitPack { std::vector<half_t> hi, lo; };
SplitPack pack_dense_split(const Folded& f, int cout, int cin, int ks, int cout_pad, int cin_pad);
// Precision float16p8: f16 image of w * 2^p and the 8-bit cross-term image; *inv = 2^-p
SplitPack pack_dense_p8(const Folded& f, int cout, int cin, int ks, int cout_pad, int cin_pad, double* inv);

// depthwise taps [k*k][ld] (layer kernel, fused block kernel)
std::vector<float> pack_depthwise_taps(const Folded& dw, int cop, int k, int ld);
// fused block's 3x3 record per channel: 9 taps, BN1 bias, BN2 bias, pad (kernels.hip: DPP depthwise)
std::vector<float> pack_depthwise_records12(const Folded& bn1, const Folded& dw, int cop, int cop_pad);
// Precision float16x3 depthwise records of a k x k depthwise (x3.hip: X3Depthwise / X3Depthwise5)
std::vector<float> pack_x3_depthwise_records(const Folded& bn1, const Folded& dw, int cop, int cop_pad, int k);

// stem kernel streams (stem.hip, kernels.h: StemArgs)
struct StemStreams { std::vector<half_t> w; std::vector<float> b; };
StemStreams pack_stem(const Folded& f, int cin, int cin_pad16);
// dense residual tower streams (restower.hip, kernels.h: ResTowerArgs); conv1 / conv2 of every block; NR = cout tiles per wave
struct ResTowerStreams { std::vector<half_t> w; std::vector<float> b; };
ResTowerStreams pack_restower(const std::vector<Folded>& conv1, const std::vector<Folded>& conv2, int C, int NR);

// One bottleneck block's contribution to the one-launch tower's per-wave streams (tower.hip, kernels.h: TowerArgs).  q = TowerArgs::fp8:
// 0 float16, 1 fp8, 2 int8 (calib: the block's calibrated maxima).  s3 / b3: the block's TowerBlockDesc arrays (s3 empty for float16).
struct TowerStreams {
    std::vector<half_t> w[4];                   // per matrix wave: f16 A fragments in consumption order
    std::vector<float> b[4];                    // per matrix wave: BN1 biases (int8: int32 bit patterns)
    std::vector<half_t> p[4];                   // per vector wave: packed f16 depthwise weights
    std::vector<uint8_t> w8e[4], w8p[4];        // fp8 / int8: per matrix wave the expand / project streams
    void append(const TowerStreams& o);
};
struct TowerBlockPack {
    TowerStreams s;
    std::vector<float> s3, b3;
    float qx_inv = 0.f, qt_inv = 0.f, escale = 0.f;
};
TowerBlockPack pack_tower_block(const BlockFold& bf, int C, int cop, int k, int q, std::pair<float, float> calib);
// a run's streams closed by their zero windows and laid out wave after wave (the kernel's windows run one window / one chunk past the end)
struct TowerImage {
    std::vector<half_t> w, p;
    std::vector<uint8_t> w8;
    std::vector<float> b;
    long long w_wave_frags = 0, e_frags = 0, b_wave_floats = 0, p_wave_bytes = 0;
};
TowerImage close_tower_streams(TowerStreams run, bool fp8);

// Precision float16x3 / float16p8: a block's images for the tower / split-board kernels (x3.hip, kernels.h: X3TowerBlock)
struct X3BlockPack {
    SplitPack w1, w3;
    std::vector<float> dw, b3;
    double w1_inv = 1.0, w3_inv = 1.0;
};
X3BlockPack pack_x3_block(const BlockFold& bf, int C, int cop, int k, int cop_pad, bool p8);

// Precision float16x3 / float16p8, "-wnet": an NTB's images for ntb_x3w_kernel (x3_wntb.cpp, kernels.h: NtbArgs).  Every 1x1 layer is the
// fragment image the layer conv reads ([cout tile][k-slab], pack_dense_split); the grouped 3x3 holds its groups only, [cout tile][tap]
// fragments over the 32 input channels of the tile's group.
struct X3NtbPack { SplitPack patch, qkv, proj, projection, mhca, mhca_proj, mlp1, mlp2; };
X3NtbPack pack_x3_ntb(const NtbFold& n);

// SE weights of block `prefix`: kind 0 none, 1 ca_se (w0 = FC1^T [C][C/2], w1 = FC2^T [C/2][C]), 2 eca_se (w0 = centre tap^T [C][C],
// b = bias); the layout of the SE / SE-gate kernels.  Throws on an unknown type.
struct SEWeights {
    int kind = 0;
    std::vector<float> w0, w1, b;
    double macs = 0;
};
SEWeights load_se(const NetFile& nf, const std::string& prefix, const std::string& type, int C);
// the same in thread order for the f16 tower (tower.hip: se_phase) and the float16x3 towers (x3.hip: x3_se_phase): first / second matrix
std::pair<std::vector<half_t>, std::vector<half_t>> pack_se_tower(const SEWeights& se);
std::pair<std::vector<float>, std::vector<float>> pack_se_x3(const SEWeights& se, int C);

// one-launch head streams (head.hip, kernels.h: HeadArgs) from the folded policy convs and value conv
struct HeadStreams { std::vector<half_t> s1, s2; std::vector<float> b1; };
HeadStreams pack_head(const Folded& policy1, const Folded& policy2, const Folded& vconv, int C, int cv, int cp);
// value head: the WDL / plys-to-end rows [4][pitch] (zeros beyond nfl); FC1 in the one-launch head's thread order; FC1 transposed
std::vector<float> pack_value_wdl(const NetFile& nf, int nfl, int pitch);
std::vector<half_t> pack_value_fc1_threads(const NetFile& nf, int nfl, int fc);
std::vector<float> pack_value_fc1_transposed(const NetFile& nf, int nfl, int fc);

}  // namespace cra
