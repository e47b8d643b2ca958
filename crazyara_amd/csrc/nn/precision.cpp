// What a net is told from outside, host code only: the precision string and the development switches of the environment.
#include <cstdlib>
#include <stdexcept>

#include "rise_net.h"

namespace cra {

namespace {
// the float16x3 forward's value head: false = conv GEMM + FC GEMM + value_final (three launches), true = value_head_kernel (one)
constexpr bool kX3ValueHeadOneLaunch = true;
}  // namespace

RiseNet::DevSwitches::DevSwitches() {
    if (const char* e = getenv("CRA_X3_CONV_DEV")) conv_dev = atoi(e);
    device_graph = getenv("CRA_DEVICE_GRAPH") != nullptr;
    lane_graph = getenv("CRA_LANE_GRAPH") != nullptr;
    lane_no_graph = getenv("CRA_LANE_NO_GRAPH") != nullptr;
    predict_copy = getenv("CRA_PREDICT_COPY") != nullptr;
    predict_zero_copy = getenv("CRA_PREDICT_ZERO_COPY") != nullptr;
    if (const char* e = getenv("CRA_LANE_LAUNCHES")) lane_launches = e[0];
    lane_sync = getenv("CRA_LANE_SYNC") != nullptr;
    if (const char* e = getenv("CRA_X3_TOWER")) x3_symmetric = e[0] == 's';
    if (const char* e = getenv("CRA_X3_SPLIT_DEV")) x3_split_dev = atoi(e);
    no_small_path = getenv("CRA_NO_SMALL_PATH") != nullptr;
    if (const char* e = getenv("CRA_SMALL_BATCH_CONV_SPLIT")) small_conv_split = atoi(e);
    tower_trace = getenv("CRA_TOWER_TRACE") != nullptr;
    x3_value_one_launch = kX3ValueHeadOneLaunch;
    if (const char* e = getenv("CRA_X3_VALUE_HEAD")) x3_value_one_launch = e[0] == 'o';
    value_head_debug = getenv("CRA_VALUE_HEAD_DEBUG") != nullptr;
    if (const char* e = getenv("CRA_VALUE_HEAD_LDS_PAD")) value_head_lds_pad = atoi(e);
    if (const char* e = getenv("CRA_VALUE_HEAD_VARIANT")) value_head_variant = atoi(e);
    x3_no_head_chain = getenv("CRA_X3_NO_HEAD_CHAIN") != nullptr;
    x3_no_tail = getenv("CRA_X3_NO_TAIL") != nullptr;
    x3_no_quad = getenv("CRA_X3_NO_QUAD") != nullptr;
    small_batch_heads_apart = getenv("CRA_SMALL_BATCH_HEADS_APART") != nullptr;
    if (const char* e = getenv("CRA_X3_HEADS_APART")) x3_heads_apart = e[0] != '0' && e[0] != 0;
    value_head_env = getenv("CRA_X3_VALUE_HEAD") != nullptr || getenv("CRA_VALUE_HEAD_VARIANT") != nullptr;
}

Precision parse_precision(const std::string& precision) {
    Precision v;
    std::string prec = precision;
    auto strip = [&](const std::string& tag) {
        if (prec.size() <= tag.size() || prec.compare(prec.size() - tag.size(), tag.size(), tag) != 0) return false;
        prec.resize(prec.size() - tag.size());
        return true;
    };
    if (strip("-3k")) v.one_launch = false;   // stem, tower and head as three launches instead of one (forward.hip); per-kernel timing and A/B reference
    if (strip("-8w")) v.thin_waves = true;
    if (strip("-1wg")) v.board_split = false;
    if (strip("-1b")) v.boards_per_wg = 1;
    else if (strip("-2b")) v.boards_per_wg = 2;
    if (strip("-wtower")) v.wtower = v.wnet = v.wblock = true;   // "-wnet", and runs of consecutive blocks in one launch (x3_wtower.cpp)
    else if (strip("-wsplit")) v.wsplit = v.wnet = v.wblock = true;   // "-wnet", and split-board blocks in nets made for few boards (x3_wsplit.cpp)
    else if (strip("-wnet")) v.wnet = v.wblock = true;   // "-wblock" plus the transformer blocks in one launch each (x3_wntb.cpp)
    else if (strip("-wblock")) v.wblock = true;    // one-launch blocks at trunk widths 128 / 192 / 224 (x3_wblock.cpp); which blocks qualify is the builder's business
    if (strip("-unfused")) v.fused = v.tower = false;
    else if (strip("-perblock")) v.tower = false;
    using M = Precision::Mode;
    // int8: the reference's calibrated reduced-precision mode (TensorRT INT8, entropy-calibrated on the plies of two recorded games:
    // tensorrtapi.cpp:334-360, chessbatchstream.cpp:44-94; UCI option Precision = int8).  Here: int8 operands in the two GEMMs of every
    // bottleneck block (v_mfma_i32_32x32x32_i8, tower.hip Q = 2), one activation step per tensor and block from a calibration pass
    // (mi_net_calibrate_int8 -> <model file>.int8calib beside the model, like TensorRT's calibration cache), one weight step per output
    // row; everything else as float16.  Round 6's study on int8 itself (scripts/studies/int8_calibration_study.py: value within 6 - 8e-3
    // of fp32, e4m3's 1 - 3e-2) replaced round 3's refusal, which rested on an e4m3 study.
    // float16x3: the fast mode that meets "logits within 1e-3 of fp32": float activations, every dense contraction as three f16 MFMAs on
    // split operands (x3.hip).  float16p8: float16x3 with the cross terms of the one-launch tower's two 1x1 GEMMs on ONE e5m2 MFMA per
    // 64 k and the residual stream in the PROJECT waves' registers (x3.hip: tower_p8_kernel): logits within 3e-4 of fp32 (emulated
    // 5e-5 ... 1.3e-4 on the parity nets)
    static const std::pair<const char*, M> kModes[] = {
        {"float16", M::Float16},   {"fp16", M::Float16},     {"half", M::Float16},      {"int8", M::Int8},
        {"fp8", M::Fp8},           {"float8", M::Fp8},       {"float32", M::Float32},   {"fp32", M::Float32},
        {"float16x3", M::Float16x3}, {"fp16x3", M::Float16x3}, {"f16x3", M::Float16x3},
        {"float16p8", M::Float16p8}, {"fp16p8", M::Float16p8}, {"f16p8", M::Float16p8}};
    for (const auto& m : kModes)
        if (prec == m.first) {
            v.mode = m.second;
            if (v.wtower && !v.x3()) throw std::invalid_argument("`-wtower` is a float16x3 kernel family (float16x3-wtower | float16p8-wtower), got '" + precision + "'");
            if (v.wtower && !v.fused) throw std::invalid_argument("`-wtower` and `-unfused` exclude each other, got '" + precision + "'");
            if (v.wsplit && !v.x3()) throw std::invalid_argument("`-wsplit` is a float16x3 kernel family (float16x3-wsplit | float16p8-wsplit), got '" + precision + "'");
            if (v.wsplit && !v.fused) throw std::invalid_argument("`-wsplit` and `-unfused` exclude each other, got '" + precision + "'");
            if (v.wsplit && !v.board_split)
                throw std::invalid_argument("`-wsplit` and `-1wg` exclude each other (several workgroups per board against one), got '" + precision + "'");
            if (v.wnet && !v.x3()) throw std::invalid_argument("`-wnet` is a float16x3 kernel family (float16x3-wnet | float16p8-wnet), got '" + precision + "'");
            if (v.wnet && !v.fused) throw std::invalid_argument("`-wnet` and `-unfused` exclude each other, got '" + precision + "'");
            if (v.wblock && !v.x3()) throw std::invalid_argument("`-wblock` is a float16x3 kernel family (float16x3-wblock | float16p8-wblock), got '" + precision + "'");
            if (v.wblock && !v.fused) throw std::invalid_argument("`-wblock` and `-unfused` exclude each other, got '" + precision + "'");
            return v;
        }
    throw std::invalid_argument("unsupported precision '" + precision + "' (float16 | float16x3 | float16p8 | float32 | fp8 | int8)");
}

}  // namespace cra
