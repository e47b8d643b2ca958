// RiseNet::build: the op list of a net's forward from its model file (the run side is rise_net.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "../chess/planes_host.h"
#include "pack.h"
#include "rise_net_impl.h"

namespace cra {

// ---- build(): the op list of the forward, stage by stage over one state (RiseNet::Builder) ----
namespace {
// which kernel family runs a bottleneck block (RiseNet::Builder::plan)
enum class Family {
    Tower,     // float16 / fp8 / int8: the one-launch tower (tower.hip), every block of the net in one run
    X3Tower,   // float16x3 / float16p8: a run of 3x3 or of 5x5 blocks in one launch (x3.hip: tower_x3_kernel, tower_p8_kernel)
    X3Split,   // float16x3 / float16p8 at small batches: a 3x3 block per launch over several workgroups per board (block_x3_split_kernel)
    Fused,     // one launch per block (kernels.hip: block_kernel; x3.hip: block_x3_kernel)
    WBlock,    // float16x3 / float16p8 with "-wblock" at 128 / 192 / 224 channels: one launch per block (x3_wblock.cpp: block_x3w_kernel)
    WSplit,    // float16x3 / float16p8 with "-wsplit" in a net made for few boards: WBlock's blocks over several workgroups per board
               // (x3_wsplit.cpp: block_x3w_split_kernel)
    WTower,    // float16x3 / float16p8 with "-wtower": WBlock's blocks, every maximal run of two or more consecutive ones in one launch
               // (x3_wtower.cpp: tower_x3w_kernel); a gated block starts a run, a run of one is a WBlock launch
    Layers,    // expand, depthwise and project as three layer launches
    Transformer,  // a NextViT transformer block: conv GEMMs and the attention kernel (Builder::transformer_block)
    WNtb       // float16x3 / float16p8 with "-wnet": a transformer block of rise_config.ntb_widths in one launch (x3_wntb.cpp: ntb_x3w_kernel)
};
struct BlockPlan {
    Family family;
    bool gate_in_kernel;   // the block's SE gate is computed in its own launch (else by an SE / SE-gate launch in front of it)
};
}  // namespace

template <typename T> struct RiseNet::Builder {
    static constexpr bool kHalf = std::is_same<T, half_t>::value;
    RiseNet& net;
    Impl& im;
    const NetFile& nf;
    const Precision& prec;
    const DevSwitches& dev;
    // the model
    int B = 0, cin = 0, C = 0, cv = 0, fc = 0, cp = 0, n_labels = 0, cin_pad = 0;
    bool wdl = false, policy_map = true, dense_blocks = false, a0_blocks = false, dense_se = false;
    bool transformers = false;        // some block is an NTB: every block and both heads run on the layer-granular kernels
    std::vector<bool> ntb;            // per block: a NextViT transformer block (model file: use_transformers)
    std::vector<std::string> se_types;
    std::vector<int> cops, ks;
    // the paths that hold for the whole net
    bool tower_ok = false;   // the one-launch f16 towers (bottleneck or dense)
    bool x3_tower = false;   // float16x3 / float16p8 tower runs
    bool x3_split = false;   // small batches: 3x3 runs one block per launch, several workgroups per board (kernels.h: X3SplitArgs)
    bool head_ok = false;    // policy + value head in one launch
    // the state: activations, SE plumbing, open runs
    T *x0 = nullptr, *cur = nullptr, *nxt = nullptr, *e = nullptr, *f = nullptr;
    // SE plumbing for the fused paths: the squeeze (per-channel sums) is produced by the previous block / tower kernel's
    // epilogue, a small gate kernel turns it into gate[b][c], and the consumer's prologue multiplies it into x while
    // loading the tile.  Inside a tower the whole SE runs in-kernel.
    float *se_pool = nullptr, *se_gate = nullptr;
    const float* pending_gate = nullptr;
    int prod_op = -1;                 // last op that produced the residual stream and can emit its channel sums
    int wblock_ops = 0;               // blocks that "-wblock" put on block_x3w_kernel (none: the precision is refused)
    int wntb_ops = 0;                 // transformer blocks that "-wnet" put on ntb_x3w_kernel
    double macs = 0;
    std::vector<TowerBlockDesc> tower_blocks;
    TowerStreams tower_streams;
    const float* tower_gate = nullptr;
    std::vector<X3TowerBlock> x3_blocks;
    int x3_run_ks = 3;                // a run is all 3x3 or all 5x5 blocks (tower_x3_roles_kernel<KS>, tower_p8_kernel<KS>)
    float* split_parts[2] = {nullptr, nullptr};
    static constexpr int kSplitMaxG = 10;
    // "-wsplit": the image sets of block_x3w_split_kernel (two alternate), the set the last launch wrote and its images per board (0: the
    // float stream in `cur` is current)
    float* wsplit_parts[2] = {nullptr, nullptr};
    int wsplit_set = 0, wsplit_g = 0;
    // "-wtower": the blocks of the open run as launch_block_x3w would take them (x, y and batch are the flush's); the first one's gate is the run's
    std::vector<BlockArgs> wrun;

    Builder(RiseNet& n, const NetFile& file) : net(n), im(*n.impl_), nf(file), prec(n.prec_), dev(n.dev_) {}
    void read_model();
    BlockPlan plan(size_t i) const;
    bool block_fused(int k) const { return prec.fused && C == 256 && !transformers && !(prec.x3() && k != 3); }   // float16x3 has a fused kernel for 3x3 blocks only
    void upload_dense(const void*& wpk, const void*& wpk_lo, const Folded& fd, int co, int ci, int k, int co_pad, int ci_pad);
    void set_conv_weights(ConvArgs& c, const Folded& fd, int co, int ci, int k, int co_pad, int ci_pad, bool p8 = false);
    ConvArgs& conv_op(const Folded& fd, const void* x, void* out, int ci, int ci_pad, int co, int k, int relu, bool p8 = false);
    void add_conv(const std::string& conv, const std::string& bn, const T* x, T* out, const T* resid, int ci, int ci_pad, int co, int k,
                  int relu, float* out_policy, bool p8 = false);
    Op se_op(const SEWeights& se);
    void add_se(Op op, bool consumer_fused);
    void stem();
    void dense_tower();
    void dense_layer_blocks();
    void bottleneck_blocks();
    void transformer_block(size_t i);
    void transformer_block_x3w(const NtbFold& n);
    void flush_tower();
    void flush_x3_run();
    void wsplit_finish();
    void flush_wrun();
    void one_launch_head();
    void policy_head();
    void softmax();
    void value_head();
    void merge_heads_x3();
    void merge_heads_small();
    void merge_forward();
};

template <typename T> void RiseNet::Builder<T>::read_model() {
    B = net.design_.batch;
    cin = int(nf.num("nb_input_channels"));
    C = int(nf.num("channels", 256));
    const int cop_init = int(nf.num("channels_operating_init"));
    const int cexp = int(nf.num("channel_expansion"));
    cv = int(nf.num("channels_value_head", 8));
    fc = int(nf.num("value_fc_size", 256));
    cp = int(nf.num("channels_policy_head"));
    wdl = nf.num("use_wdl") != 0 && nf.num("use_plys_to_end") != 0;
    std::vector<std::string> kernels = nf.list("kernels");
    se_types = nf.list("se_types");
    if (kernels.empty() || kernels.size() != se_types.size()) throw std::runtime_error("kernels/se_types mismatch in model file");
    // residual block family: RiseV3's mobile bottleneck (default), ClassicalResidualBlock (builder_util.py:401-434) or
    // AlphaZeroResnet's ResidualBlock (a0_resnet.py:72-107); the last two are towers of dense 3x3 convolutions
    const std::string conv_block = nf.str("conv_block", "mobile_bottlekneck_res_block");
    a0_blocks = conv_block == "a0_res_block";
    dense_blocks = conv_block == "classical_res_block" || a0_blocks;
    if (!dense_blocks && conv_block != "mobile_bottlekneck_res_block") throw std::runtime_error("unsupported conv_block '" + conv_block + "'");
    // SE inside dense residual blocks (ClassicalResidualBlock(se_type), builder_util.py:401-434: gate on the block INPUT, hard-sigmoid;
    // AlphaZero ResidualBlock(use_se), a0_resnet.py:72-107: gate on the body OUTPUT, plain sigmoid): such nets run their blocks on the
    // layer kernels (conv GEMM + SE kernel), not on the one-launch dense tower
    if (dense_blocks)
        for (const std::string& t : se_types) dense_se |= !(t == "none" || t.empty());
    // (every kernel specialised for a width needs C = 256; the mobile-bottleneck layer path takes any multiple of 32, AlphaVile's 224 among
    // them -- the dense families keep the multiples of 64 they are tested at)
    if (dense_blocks && (C % 64 != 0 || C > 512)) throw std::runtime_error("channels must be a multiple of 64 and <= 512");
    if (C % 32 != 0 || C > 512) throw std::runtime_error("channels must be a multiple of 32 and <= 512");
    if (fc > 256 && fc % 256 != 0) throw std::runtime_error("unsupported value_fc_size");

    net.design_.nb_input_channels = cin;
    // _PolicyHead form (builder_util.py:206-243): policy map (the P planes, channel-major) or flat labels (Linear on top)
    policy_map = nf.num("select_policy_from_plane", 1) != 0;
    n_labels = int(nf.num("n_labels", 0));
    if (!policy_map && (n_labels <= 0 || (cp * kSquares) % 32 != 0)) throw std::runtime_error("flat policy head needs n_labels and P*64 % 32 == 0");
    net.design_.nb_policy = policy_map ? cp * kSquares : n_labels;
    net.design_.nb_aux = wdl ? 4 : 0;
    cin_pad = round_up(cin, 32);
    im.cin_pad = cin_pad;

    // C_op schedule: rise_mobile_v3.py:36-78 (kernel_5_channel_ratio=None)
    int cop_run = cop_init, cop_max = 32;
    const std::vector<std::string> cop_list = nf.list("channels_operating");     // imported models carry the widths they were found with
    if (!cop_list.empty() && cop_list.size() != kernels.size()) throw std::runtime_error("channels_operating/kernels mismatch in model file");
    for (size_t i = 0; i < kernels.size(); ++i) {
        const int k = std::stoi(kernels[i]);
        if (k != 3 && k != 5) throw std::runtime_error("unsupported depthwise kernel size " + kernels[i]);
        const int c = !cop_list.empty() ? std::stoi(cop_list[i]) : k == 5 ? cop_run - 32 * int(i / 2) : cop_run;
        if (c % 32 != 0 || c <= 0) throw std::runtime_error("channels_operating must be a positive multiple of 32");
        cops.push_back(c);
        ks.push_back(k);
        cop_max = std::max(cop_max, c);
        cop_run += cexp;
    }
    // NextViT transformer blocks (RiseV3(use_transformers), AlphaVile): the scratch tiles e / f also hold q|k|v (3 D < 3 C channels) and
    // the Mlp's hidden layer
    const std::vector<std::string> tr_list = nf.list("use_transformers");
    if (!tr_list.empty() && tr_list.size() != kernels.size()) throw std::runtime_error("use_transformers/kernels mismatch in model file");
    ntb.assign(kernels.size(), false);
    for (size_t i = 0; i < tr_list.size(); ++i) {
        const std::string& t = tr_list[i];
        ntb[i] = !(t == "0" || t == "none" || t == "False" || t == "false" || t.empty());
        if (!ntb[i]) continue;
        if (dense_blocks) throw std::runtime_error("transformer blocks are supported in RiseV3 mobile-bottleneck nets only");
        transformers = true;
        const std::string p = "body_spatial." + std::to_string(i + 1) + ".mlp.conv1.weight";
        cop_max = std::max(cop_max, 3 * C);
        if (nf.has(p)) cop_max = std::max(cop_max, int(nf.get(p).shape[0]));
    }

    tower_ok = prec.tower && prec.fused && kHalf && C == 256 && !dense_se && !transformers;
    if (prec.fp8_tower() && (!tower_ok || dense_blocks))
        throw std::runtime_error("Precision fp8 runs on the one-launch bottleneck tower only (256-channel RISE nets): use float16 for this model");
    x3_tower = prec.x3() && prec.tower && prec.fused && C == 256 && !transformers;
    x3_split = x3_tower && prec.board_split && B <= kBoardSplitMaxBatch;
    // value heads with fewer than 8 channels (AlphaZeroResnet: 4) run as 8 with zero rows: ReLU(0) = 0 meets zero FC weights
    head_ok = tower_ok && policy_map && cv >= 1 && cv <= 8 && cp <= 96 && (wdl || fc == 256);

    // ---- device buffers ----
    net.d_desc_ = im.dalloc(size_t(B) * sizeof(BoardDesc));
    net.d_planes_ = static_cast<float*>(im.dalloc(size_t(B) * cin * kSquares * sizeof(float)));
    net.d_value_ = static_cast<float*>(im.dalloc(size_t(B) * sizeof(float)));
    net.d_probs_ = static_cast<float*>(im.dalloc(size_t(B) * net.design_.nb_policy * sizeof(float)));
    net.d_logits_ = static_cast<float*>(im.dalloc(size_t(B) * net.design_.nb_policy * sizeof(float)));
    net.d_aux_ = wdl ? static_cast<float*>(im.dalloc(size_t(B) * 4 * sizeof(float))) : nullptr;
    x0 = static_cast<T*>(im.dalloc(size_t(B) * kSquares * cin_pad * sizeof(T)));
    cur = static_cast<T*>(im.dalloc(size_t(B) * kSquares * C * sizeof(T)));
    nxt = static_cast<T*>(im.dalloc(size_t(B) * kSquares * C * sizeof(T)));
    e = static_cast<T*>(im.dalloc(size_t(B) * kSquares * cop_max * sizeof(T)));
    f = static_cast<T*>(im.dalloc(size_t(B) * kSquares * cop_max * sizeof(T)));
}

// the one place that decides which family runs bottleneck block i and where its SE gate is computed
template <typename T> BlockPlan RiseNet::Builder<T>::plan(size_t i) const {
    const int k = ks[i];
    if (ntb[i]) {
        if (prec.wnet && prec.x3()) {                        // "-wnet": the widths ntb_x3w_kernel is made for; any other NTB keeps its nine launches
            const std::string p = "body_spatial." + std::to_string(i + 1);
            if (nf.has(p + ".patch_embed.conv.weight") && nf.has(p + ".mlp.conv1.weight")) {
                const int D = int(nf.get(p + ".patch_embed.conv.weight").shape[0]), H = int(nf.get(p + ".mlp.conv1.weight").shape[0]);
                if (ntb_x3w_supports(C, D, C - D, H)) return {Family::WNtb, false};
            }
        }
        return {Family::Transformer, false};
    }
    // "-wblock": every other block of a 128 / 192 / 224-channel net, also between transformer blocks; the gate comes from the launches in front
    // "-wsplit": the same blocks over several workgroups per board in a net made for few boards (a larger net builds "-wnet"'s list)
    // "-wtower": the same blocks, consecutive ones in one launch (bottleneck_blocks, flush_wrun), whatever the batch the net is made for
    if (prec.wblock && prec.x3() && !dense_blocks && block_x3w_supports(C, k))
        return {prec.wtower ? Family::WTower : prec.wsplit && B <= kBoardSplitMaxBatch ? Family::WSplit : Family::WBlock, false};
    if (tower_ok) return {Family::Tower, i > 0};          // 3x3 and 5x5 blocks in one run; the run's first gate comes from an SE launch
    if (x3_tower) {
        // the 5x5 blocks (RISEv3.3) run in tower launches of their own (tower_*_kernel<5>); small batches run 3x3 blocks split-board (float16x3
        // images, own gate); float16p8 also computes a run's first gate in the launch, float16x3 takes it from an SE launch
        const bool split = x3_split && k == 3;
        return {split ? Family::X3Split : Family::X3Tower, split || prec.p8() || (i > 0 && ks[i - 1] == k)};
    }
    return {block_fused(k) ? Family::Fused : Family::Layers, false};
}

// packed A-fragment images of a dense layer: T, or the f16 hi / lo pair of Precision float16x3
template <typename T>
void RiseNet::Builder<T>::upload_dense(const void*& wpk, const void*& wpk_lo, const Folded& fd, int co, int ci, int k, int co_pad, int ci_pad) {
    if (prec.x3()) {
        SplitPack sp = pack_dense_split(fd, co, ci, k, co_pad, ci_pad);
        wpk = im.upload(sp.hi);
        wpk_lo = im.upload(sp.lo);
    } else {
        wpk = im.upload(pack_dense<T>(fd, co, ci, k, co_pad, ci_pad));
    }
}

template <typename T>
void RiseNet::Builder<T>::set_conv_weights(ConvArgs& c, const Folded& fd, int co, int ci, int k, int co_pad, int ci_pad, bool p8) {
    if (p8 && prec.p8() && k == 3 && ci_pad % 128 == 0) {     // Precision float16p8: the policy head's 3x3 convs (x3.hip: conv3x3_p8_kernel)
        double inv = 1.0;
        SplitPack sp = pack_dense_p8(fd, co, ci, k, co_pad, ci_pad, &inv);
        c.wpk = im.upload(sp.hi);
        c.wpk_lo = im.upload(sp.lo);
        c.p8 = 1;
        c.acc_scale = float(inv);
    } else {
        upload_dense(c.wpk, c.wpk_lo, fd, co, ci, k, co_pad, ci_pad);
    }
}

// a conv-GEMM launch over the B boards; the caller sets what differs (other output layouts, a GEMM over the batch)
template <typename T>
ConvArgs& RiseNet::Builder<T>::conv_op(const Folded& fd, const void* x, void* out, int ci, int ci_pad, int co, int k, int relu, bool p8) {
    const int co_pad = round_up(co, 16);
    Op op;
    op.kind = OpKind::Conv;
    ConvArgs& c = op.conv;
    c.x = x;
    set_conv_weights(c, fd, co, ci, k, co_pad, ci_pad, p8);
    c.bias = im.upload_d2f(fd.b, co_pad);
    c.out = out;
    c.batch = B;
    c.cin = ci_pad;
    c.cout_pad = c.cout_ld = co_pad;
    c.cout_real = co;
    c.ks = k;
    c.relu = relu;
    im.ops.push_back(op);
    return im.ops.back().conv;
}

template <typename T>
void RiseNet::Builder<T>::add_conv(const std::string& conv, const std::string& bn, const T* x, T* out, const T* resid, int ci, int ci_pad,
                                   int co, int k, int relu, float* out_policy, bool p8) {
    ConvArgs& c = conv_op(fold_bn(nf, conv, bn), x, out_policy ? static_cast<void*>(out_policy) : static_cast<void*>(out), ci, ci_pad, co, k, relu, p8);
    c.resid = resid;
    c.out_policy_f32 = out_policy ? 1 : 0;
    macs += double(kSquares) * ci * co * k * k;
}

// an SE / SE-gate launch's weights (kind and target are the caller's)
template <typename T> Op RiseNet::Builder<T>::se_op(const SEWeights& se) {
    Op op;
    op.se_kind = se.kind;
    op.w0 = im.upload(se.w0);
    if (se.kind == 1) op.w1 = im.upload(se.w1);
    else op.b0 = im.upload(se.b);
    op.C = C;
    return op;
}

template <typename T> void RiseNet::Builder<T>::add_se(Op op, bool consumer_fused) {
    if (consumer_fused && prod_op >= 0) {
        if (!se_pool) {
            se_pool = static_cast<float*>(im.dalloc(size_t(B) * C * sizeof(float)));
            se_gate = static_cast<float*>(im.dalloc(size_t(B) * C * sizeof(float)));
        }
        if (im.ops[prod_op].kind == OpKind::Tower) im.ops[prod_op].tw.pool_out = se_pool;
        else if (im.ops[prod_op].kind == OpKind::TowerX3W) im.ops[prod_op].wt.pool_out = se_pool;
        else if (im.ops[prod_op].kind == OpKind::X3WSplitFinish) im.ops[prod_op].ws.blk.pool_out = se_pool;
        else im.ops[prod_op].blk.pool_out = se_pool;
        op.kind = OpKind::SEGate;
        op.x = se_pool;
        op.y = se_gate;
        pending_gate = se_gate;
    } else {
        op.kind = OpKind::SE;      // in-place scaling kernel (input produced by the stem conv, or layer-granular path)
        op.y = cur;
    }
    im.ops.push_back(op);
}

template <typename T> void RiseNet::Builder<T>::stem() {
    const int cin_pad16 = std::max(48, round_up(cin, 16));
    if (prec.tower && prec.fused && kHalf && C == 256 && cin_pad16 <= 96 && !transformers) {
        // stem kernel: planes -> conv3x3 + BN + ReLU -> NHWC f16 in one launch (stem.hip)
        const StemStreams ss = pack_stem(fold_bn(nf, "body_spatial.0.body.0", "body_spatial.0.body.1"), cin, cin_pad16);
        Op op;
        op.kind = OpKind::Stem;
        op.st.planes = net.d_planes_;
        op.st.x = cur;
        op.st.stem_w = im.upload(ss.w);
        op.st.stem_b = im.upload(ss.b);
        op.st.stem_wave_frags = 9 * (cin_pad16 / 16) + 16;
        op.st.cin = cin;
        op.st.cin_pad = cin_pad16;
        op.st.batch = B;
        im.ops.push_back(op);
        macs += double(kSquares) * cin * C * 9;
        return;
    }
    if (!prec.x3()) {   // input layout transform (Precision float16x3: the stem conv reads the planes itself)
        Op op;
        op.kind = OpKind::PlanesToAct;
        op.x = net.d_planes_;
        op.y = x0;
        op.C = cin;
        im.ops.push_back(op);
    }
    add_conv("body_spatial.0.body.0", "body_spatial.0.body.1", x0, cur, nullptr, cin, cin_pad, C, 3, true, nullptr);   // _Stem
    if (prec.x3()) {
        im.ops.back().from_planes = true;
        im.ops.back().conv.planes_c = cin;
        if (x3_split) im.ops.back().conv.few_boards = dev.small_conv_split;      // the stem's couts over several workgroups per board
    }
}

template <typename T> void RiseNet::Builder<T>::dense_tower() {
    // all blocks in one launch (restower.hip; stream layouts in kernels.h: ResTowerArgs)
    // wave shape (restower.hip): 4 fat waves of 64 couts by default, "-8w" = 8 waves of 32 couts (the first version)
    const int NR = prec.thin_waves ? 1 : 2;
    std::vector<Folded> f1s, f2s;
    for (size_t i = 0; i < cops.size(); ++i) {
        const std::string p = "body_spatial." + std::to_string(i + 1);
        f1s.push_back(fold_bn(nf, p + ".body.0", p + ".body.1"));
        f2s.push_back(fold_bn(nf, p + ".body.3", p + ".body.4"));
    }
    const ResTowerStreams rs = pack_restower(f1s, f2s, C, NR);
    Op op;
    op.kind = OpKind::ResTower;
    op.rt.x = cur;
    op.rt.y = nxt;
    op.rt.wstream = im.upload(rs.w);
    op.rt.bstream = im.upload(rs.b);
    op.rt.wstream_wave_frags = (long long)(cops.size() * 2 * 9 * 16 * NR + 16);
    op.rt.bstream_wave_floats = (long long)(cops.size() * 64 * NR);
    op.rt.cout_tiles_per_wave = NR;
    op.rt.nblocks = int(cops.size());
    op.rt.relu_after_add = a0_blocks ? 1 : 0;
    op.rt.batch = B;
    // two boards per workgroup halve the weight stream per board but fill only B/2 CUs: from 512 boards on, or on request
    // (two evaluator lanes of 256 keep 512 boards in flight)
    op.rt.boards_per_workgroup = prec.boards_per_wg ? prec.boards_per_wg : (B >= 512 ? 2 : 1);
    im.ops.push_back(op);
    macs += double(cops.size()) * 2.0 * kSquares * C * C * 9;
    std::swap(cur, nxt);
}

template <typename T> void RiseNet::Builder<T>::dense_layer_blocks() {
    // gate of a dense block as an in-place SE op on `target` (+ optional shortcut `res`: target = relu(res + target * gate))
    auto dense_se_op = [&](const SEWeights& se, T* target, const T* res, bool plain_sigmoid) {
        Op op = se_op(se);
        op.kind = OpKind::SE;
        op.y = target;
        op.x = res;
        macs += se.macs;
        if (plain_sigmoid) op.se_kind |= 16;
        im.ops.push_back(op);
    };
    for (size_t i = 0; i < cops.size(); ++i) {
        // x -> conv3x3 + BN + ReLU -> conv3x3 + BN -> classical: x + ReLU(.)   a0: ReLU(x + .)
        const std::string p = "body_spatial." + std::to_string(i + 1);
        const SEWeights se = load_se(nf, p, se_types[i], C);
        if (se.kind && !a0_blocks) dense_se_op(se, cur, nullptr, false);       // classical: x = se(x) first (builder_util.py:431-433)
        add_conv(p + ".body.0", p + ".body.1", cur, nxt, nullptr, C, C, C, 3, 1, nullptr);
        T* out = e;                                   // e: scratch of at least C channels per square
        if (se.kind && a0_blocks) {
            // out = BN(conv(.)) without shortcut, then out = relu(x + se(out)) in the gate kernel (a0_resnet.py:104-107)
            add_conv(p + ".body.3", p + ".body.4", nxt, out, nullptr, C, C, C, 3, 0, nullptr);
            dense_se_op(se, out, cur, true);
        } else {
            add_conv(p + ".body.3", p + ".body.4", nxt, out, cur, C, C, C, 3, a0_blocks ? 1 : 2, nullptr);
        }
        // keep (cur, nxt) = (block output, scratch): rotate the three buffers
        T* old = cur;
        cur = out;
        e = old;
    }
}

template <typename T> void RiseNet::Builder<T>::bottleneck_blocks() {
    for (size_t i = 0; i < cops.size(); ++i) {
        const std::string p = "body_spatial." + std::to_string(i + 1);
        const int cop = cops[i], k = ks[i];
        const BlockPlan bp = plan(i);
        if (bp.family != Family::WSplit) wsplit_finish();        // whatever else runs here reads the float stream
        if (bp.family != Family::WTower) flush_wrun();           // a transformer block or any other family ends a run
        if (bp.family == Family::Transformer || bp.family == Family::WNtb) {
            if (bp.family == Family::WNtb) transformer_block_x3w(fold_ntb(nf, p, C));
            else transformer_block(i);
            continue;
        }
        const bool x3_family = bp.family == Family::X3Tower || bp.family == Family::X3Split;
        if (!x3_blocks.empty() && x3_run_ks != k) flush_x3_run();
        TowerBlockDesc td{};
        X3TowerBlock xb{};
        const SEWeights se = load_se(nf, p, se_types[i], C);
        if (se.kind && bp.gate_in_kernel && bp.family == Family::Tower) {
            const auto pk = pack_se_tower(se);
            td.se_kind = se.kind;
            td.se_w1 = im.upload(pk.first);
            if (se.kind == 1) td.se_w2 = im.upload(pk.second);
            else td.se_b = im.upload(se.b);
        } else if (se.kind && bp.gate_in_kernel) {
            const auto pk = pack_se_x3(se, C);
            xb.se_kind = se.kind;
            xb.se_w1t = im.upload(pk.first);
            if (se.kind == 1) xb.se_w2t = im.upload(pk.second);
            else xb.se_b = im.upload(se.b);
        } else if (se.kind) {
            // (a gated split-board block reads the float stream: the finish launch in front of it leaves the stream's channel sums as the
            // one-launch block before it would have, its gate is WBlock's; behind the stem or a transformer block: the in-place SE launch)
            if (bp.family == Family::WSplit) wsplit_finish();
            // (only a run's first block may be gated: the run in front of a gated block ends here, its last block leaves the channel sums)
            if (bp.family == Family::WTower) flush_wrun();
            add_se(se_op(se), bp.family == Family::Fused || bp.family == Family::WBlock || bp.family == Family::WSplit || bp.family == Family::WTower);
        }
        macs += se.macs;
        if (bp.family == Family::Tower) {
            // residual tower: this block joins the current run of blocks (one launch per run, kernels.h: TowerArgs)
            if (prec.int8() && i >= net.int8_calib_.size()) throw std::runtime_error("INT8 calibration file holds fewer blocks than the model");
            const TowerBlockPack pk = pack_tower_block(fold_block(nf, p), C, cop, k, prec.int8() ? 2 : prec.fp8_tower() ? 1 : 0,
                                                       prec.int8() ? net.int8_calib_[i] : std::pair<float, float>{});
            if (!pk.s3.empty()) td.s3 = im.upload(pk.s3);
            td.b3 = im.upload(pk.b3);
            td.qx_inv = pk.qx_inv;
            td.qt_inv = pk.qt_inv;
            td.escale = pk.escale;
            td.cop_pad = round_up(cop, 128);
            td.ks = k;
            if (tower_blocks.empty()) {
                tower_gate = pending_gate;     // gate computed by the launches before this run (or none)
                pending_gate = nullptr;
            }
            tower_blocks.push_back(td);
            tower_streams.append(pk.s);
        } else if (x3_family) {
            const int cop_pad = round_up(cop, block_x3_chunk_channels());
            const X3BlockPack pk = pack_x3_block(fold_block(nf, p), C, cop, k, cop_pad, prec.p8() && bp.family != Family::X3Split);
            xb.w1pk = im.upload(pk.w1.hi);
            xb.w1pk_lo = im.upload(pk.w1.lo);
            xb.w3pk = im.upload(pk.w3.hi);
            xb.w3pk_lo = im.upload(pk.w3.lo);
            xb.dwpk = im.upload(pk.dw);
            xb.b3 = im.upload(pk.b3);
            xb.w1_inv = float(pk.w1_inv);                                  // float16p8: the accumulators run in the weights' scales
            xb.w3_inv = float(pk.w3_inv);
            xb.w3_scale = float(1.0 / pk.w3_inv);
            xb.cop_pad = cop_pad;
            xb.tail = cop_pad - cop >= 64 ? 1 : 0;                         // the last chunk's upper half is padding (tower_x3_tail_kernel)
            if (x3_blocks.empty()) x3_run_ks = k;
            x3_blocks.push_back(xb);
        } else if (bp.family == Family::Fused) {
            // fused bottleneck block: expand -> depthwise -> project -> +x in one launch (kernels.hip: block_kernel; x3.hip: block_x3_kernel)
            const int cop_pad = round_up(cop, prec.x3() ? block_x3_chunk_channels() : block_chunk_channels<T>());
            const BlockFold bf = fold_block(nf, p);
            Op op;
            op.kind = OpKind::Block;
            BlockArgs& ba = op.blk;
            ba.x = cur;
            ba.y = nxt;
            upload_dense(ba.w1pk, ba.w1pk_lo, bf.expand, cop, C, 1, cop_pad, C);
            upload_dense(ba.w3pk, ba.w3pk_lo, bf.project, C, cop, 1, C, cop_pad);
            ba.b1 = im.upload_d2f(bf.expand.b, cop_pad);
            ba.wdw = im.upload(pack_depthwise_taps(bf.dw, cop, k, cop_pad));
            ba.b2 = im.upload_d2f(bf.dw.b, cop_pad);
            ba.b3 = im.upload_d2f(bf.project.b, C);
            ba.batch = B;
            ba.C = C;
            ba.cop_pad = cop_pad;
            ba.ks = k;
            if (k == 3)    // per-channel record for the DPP depthwise kernel: 9 taps, BN1 bias, BN2 bias, pad (float16x3: its tile layout)
                ba.dwpk = im.upload(prec.x3() ? pack_x3_depthwise_records(bf.expand, bf.dw, cop, cop_pad, 3)
                                             : pack_depthwise_records12(bf.expand, bf.dw, cop, cop_pad));
            ba.gate = pending_gate;
            pending_gate = nullptr;
            prod_op = int(im.ops.size());
            im.ops.push_back(op);
            std::swap(cur, nxt);
        } else if (bp.family == Family::WBlock) {
            // block_x3w_kernel: C_op padded to 64 (a last chunk of 64 channels runs as such), float16x3 images in both modes
            const int cop_pad = round_up(cop, 64);
            const X3BlockPack pk = pack_x3_block(fold_block(nf, p), C, cop, k, cop_pad, false);
            Op op;
            op.kind = OpKind::BlockX3W;
            BlockArgs& ba = op.blk;
            ba.x = cur;
            ba.y = nxt;
            ba.w1pk = im.upload(pk.w1.hi);
            ba.w1pk_lo = im.upload(pk.w1.lo);
            ba.w3pk = im.upload(pk.w3.hi);
            ba.w3pk_lo = im.upload(pk.w3.lo);
            ba.dwpk = im.upload(pk.dw);
            ba.b3 = im.upload(pk.b3);
            ba.batch = B;
            ba.C = C;
            ba.cop_pad = cop_pad;
            ba.ks = k;
            ba.gate = pending_gate;
            pending_gate = nullptr;
            prod_op = int(im.ops.size());
            im.ops.push_back(op);
            ++wblock_ops;
            std::swap(cur, nxt);
        } else if (bp.family == Family::WTower) {
            // WBlock's images and arguments; the launch is flush_wrun's
            const int cop_pad = round_up(cop, 64);
            const X3BlockPack pk = pack_x3_block(fold_block(nf, p), C, cop, k, cop_pad, false);
            BlockArgs ba{};
            ba.w1pk = im.upload(pk.w1.hi);
            ba.w1pk_lo = im.upload(pk.w1.lo);
            ba.w3pk = im.upload(pk.w3.hi);
            ba.w3pk_lo = im.upload(pk.w3.lo);
            ba.dwpk = im.upload(pk.dw);
            ba.b3 = im.upload(pk.b3);
            ba.batch = B;
            ba.C = C;
            ba.cop_pad = cop_pad;
            ba.ks = k;
            ba.gate = pending_gate;            // (set for an empty run only: a gated block has just ended the run in front of it)
            pending_gate = nullptr;
            wrun.push_back(ba);
            ++wblock_ops;
        } else if (bp.family == Family::WSplit) {
            // block_x3w_split_kernel: WBlock's images; the block reads the images of the launch before it (or the float stream: the first
            // block, behind a transformer block, a gated block) and writes the other image set.  G and gin are those of a whole batch;
            // a call of fewer boards takes its own (launch_op).
            const int cop_pad = round_up(cop, 64);
            const X3BlockPack pk = pack_x3_block(fold_block(nf, p), C, cop, k, cop_pad, false);
            if (!wsplit_parts[0]) {
                int max_chunks = 1;
                for (size_t q = 0; q < cops.size(); ++q)
                    if (!ntb[q]) max_chunks = std::max(max_chunks, x3w_split_chunks(round_up(cops[q], 64)));
                const size_t images = size_t(std::min(max_chunks, int(kX3WSplitMaxG)));       // G <= that, and a call has at most B boards
                for (auto& q : wsplit_parts) q = static_cast<float*>(im.dalloc(size_t(B) * images * kSquares * C * sizeof(float)));
            }
            Op op;
            op.kind = OpKind::BlockX3WSplit;
            BlockArgs& ba = op.ws.blk;
            ba.w1pk = im.upload(pk.w1.hi);
            ba.w1pk_lo = im.upload(pk.w1.lo);
            ba.w3pk = im.upload(pk.w3.hi);
            ba.w3pk_lo = im.upload(pk.w3.lo);
            ba.dwpk = im.upload(pk.dw);
            ba.b3 = im.upload(pk.b3);
            ba.batch = B;
            ba.C = C;
            ba.cop_pad = cop_pad;
            ba.ks = k;
            ba.gate = pending_gate;
            pending_gate = nullptr;
            op.ws.stream_in = wsplit_g == 0 ? 1 : 0;
            op.ws.x_parts = wsplit_g == 0 ? reinterpret_cast<const float*>(cur) : wsplit_parts[wsplit_set];
            op.ws.gin = std::max(1, wsplit_g);
            wsplit_set ^= 1;
            op.ws.y_parts = wsplit_parts[wsplit_set];
            op.ws.G = x3w_split_shares(cop_pad, B, net.cu_count_);
            wsplit_g = op.ws.G;
            prod_op = -1;                  // (channel sums come from the finish launch, wsplit_finish)
            im.ops.push_back(op);
            ++wblock_ops;
        } else {
            add_conv(p + ".body.0", p + ".body.1", cur, e, nullptr, C, C, cop, 1, true, nullptr);   // 1x1 expand + BN + ReLU
            {   // depthwise k x k + BN + ReLU
                Folded fd = fold_bn(nf, p + ".body.3", p + ".body.4");
                Op op;
                op.kind = OpKind::Depthwise;
                op.x = e;
                op.y = f;
                op.w0 = im.upload(pack_depthwise_taps(fd, cop, k, cop));
                op.b0 = im.upload_d2f(fd.b);
                op.C = cop;
                op.ks = k;
                im.ops.push_back(op);
                macs += double(kSquares) * cop * k * k;
            }
            add_conv(p + ".body.6", p + ".body.7", f, nxt, cur, cop, cop, C, 1, false, nullptr);    // 1x1 project + BN + residual
            std::swap(cur, nxt);
            prod_op = -1;                  // the residual stream now comes from a layer kernel: nobody emits its channel sums
            continue;
        }
        macs += double(kSquares) * cop * (2.0 * C + k * k);
    }
    flush_tower();
    flush_x3_run();
    wsplit_finish();
    flush_wrun();
}

// "-wtower": the open run cur -> nxt.  One block: "-wblock"'s launch, unchanged; two or more: one tower_x3w_kernel launch over a device array of
// the blocks' records (an upload of the net's, freed with it).  Either can emit the stream's channel sums (add_se).
template <typename T> void RiseNet::Builder<T>::flush_wrun() {
    if (wrun.empty()) return;
    Op op;
    if (wrun.size() == 1) {
        op.kind = OpKind::BlockX3W;
        op.blk = wrun[0];
        op.blk.x = cur;
        op.blk.y = nxt;
    } else {
        std::vector<X3WTowerBlock> recs;
        for (const BlockArgs& ba : wrun) {
            if (ba.gate && &ba != &wrun[0]) throw std::logic_error("flush_wrun: a gated block inside a run");
            recs.push_back(X3WTowerBlock{ba.w1pk, ba.w1pk_lo, ba.w3pk, ba.w3pk_lo, ba.dwpk, ba.b3, ba.cop_pad, ba.ks});
        }
        op.kind = OpKind::TowerX3W;
        op.wt.x = reinterpret_cast<const float*>(cur);
        op.wt.y = reinterpret_cast<float*>(nxt);
        op.wt.blocks = im.upload(recs);
        op.wt.nblocks = int(recs.size());
        op.wt.gate = wrun[0].gate;
        op.wt.batch = B;
        op.wt.C = C;
    }
    prod_op = int(im.ops.size());
    im.ops.push_back(op);
    wrun.clear();
    std::swap(cur, nxt);
}

// "-wsplit": the images of the last split-board block -> the float stream `cur`, in front of whatever reads the stream.  It can emit the
// stream's channel sums (add_se) as a one-launch block does.
template <typename T> void RiseNet::Builder<T>::wsplit_finish() {
    if (wsplit_g == 0) return;
    Op fin;
    fin.kind = OpKind::X3WSplitFinish;
    fin.ws.x_parts = wsplit_parts[wsplit_set];
    fin.ws.gin = wsplit_g;
    fin.ws.blk.y = cur;
    fin.ws.blk.C = C;
    fin.ws.blk.batch = B;
    prod_op = int(im.ops.size());
    im.ops.push_back(fin);
    wsplit_g = 0;
}

// NTB (next_vit_official_modules.py:267-335) on the layer kernels.  The block's C-wide tile xs (= nxt) holds the E_MHSA part in channels
// [0, D) and the MHCA part in [D, C): the concat is where the convs write (ConvArgs::cout_ld = C) and read (ConvArgs::x_ld = C), no copy.
//   patch_embed    cur -> xs[0, D)                   conv1x1 + BN
//   q | k | v      xs[0, D) -> e [3D]                one GEMM, norm1 folded in, bias
//   attention      e -> f [D]                        attention.hip
//   proj           f -> xs[0, D), + xs[0, D)         bias; the residual is the patch-embed output (in place: each element is read and
//                                                    written by the same lane)
//   projection     xs[0, D) -> xs[D, C)              conv1x1 + BN: u
//   MHCA           xs[D, C) -> f [M]                 block-diagonal 3x3 + BN + ReLU
//                  f -> xs[D, C), + u                conv1x1
//   Mlp            xs -> e [H] -> cur, + xs          norm2 folded into conv1; ReLU; conv2 (the block input is dead by then)
template <typename T> void RiseNet::Builder<T>::transformer_block(size_t i) {
    const NtbFold n = fold_ntb(nf, "body_spatial." + std::to_string(i + 1), C);
    const int D = n.D, M = n.M, H = n.H;
    T* xs = nxt;
    conv_op(n.patch, cur, xs, C, C, D, 1, 0).cout_ld = C;
    conv_op(n.qkv, xs, e, D, D, 3 * D, 1, 0).x_ld = C;
    {
        Op op;
        op.kind = OpKind::Attention;
        op.x = e;
        op.y = f;
        op.C = D;
        im.ops.push_back(op);
    }
    {
        ConvArgs& c = conv_op(n.proj, f, xs, D, D, D, 1, 0);
        c.resid = xs;
        c.cout_ld = C;
    }
    {
        ConvArgs& c = conv_op(n.projection, xs, xs + D, D, D, M, 1, 0);
        c.x_ld = C;
        c.cout_ld = C;
    }
    conv_op(n.mhca, xs + D, f, M, M, M, 3, 1).x_ld = C;
    {
        ConvArgs& c = conv_op(n.mhca_proj, f, xs + D, M, M, M, 1, 0);
        c.resid = xs + D;
        c.cout_ld = C;
    }
    conv_op(n.mlp1, xs, e, C, C, H, 1, 1);
    conv_op(n.mlp2, e, cur, H, H, C, 1, 0).resid = xs;
    macs += n.macs;
    prod_op = -1;
}

// NTB in one launch ("-wnet", x3_wntb.cpp): fold_ntb's layers as ntb_x3w_kernel's images; cur -> nxt.  Like the layer form it emits no
// channel sums: a gated block behind it takes its squeeze from an SE launch.
template <typename T> void RiseNet::Builder<T>::transformer_block_x3w(const NtbFold& n) {
    const X3NtbPack pk = pack_x3_ntb(n);
    Op op;
    op.kind = OpKind::NtbX3W;
    NtbArgs& a = op.ntb;
    a.x = reinterpret_cast<const float*>(cur);
    a.y = reinterpret_cast<float*>(nxt);
    a.batch = B;
    a.C = C;
    a.D = n.D;
    a.M = n.M;
    a.H = n.H;
    auto layer = [&](const SplitPack& sp, const Folded& fd, int co) { return NtbLayer{im.upload(sp.hi), im.upload(sp.lo), im.upload_d2f(fd.b, size_t(co))}; };
    a.patch = layer(pk.patch, n.patch, n.D);
    a.qkv = layer(pk.qkv, n.qkv, 3 * n.D);
    a.proj = layer(pk.proj, n.proj, n.D);
    a.projection = layer(pk.projection, n.projection, n.M);
    a.mhca = layer(pk.mhca, n.mhca, n.M);
    a.mhca_proj = layer(pk.mhca_proj, n.mhca_proj, n.M);
    a.mlp1 = layer(pk.mlp1, n.mlp1, n.H);
    a.mlp2 = layer(pk.mlp2, n.mlp2, C);
    im.ops.push_back(op);
    macs += n.macs;
    ++wntb_ops;
    prod_op = -1;
    std::swap(cur, nxt);
}

template <typename T> void RiseNet::Builder<T>::flush_tower() {
    if (tower_blocks.empty()) return;
    Op op;
    op.kind = OpKind::Tower;
    op.tw.x = cur;
    op.tw.y = nxt;
    op.tw.blocks = im.upload(tower_blocks);
    op.tw.nblocks = int(tower_blocks.size());
    const TowerImage ti = close_tower_streams(std::move(tower_streams), prec.fp8_tower());
    tower_streams = TowerStreams();
    if (prec.fp8_tower()) {
        op.tw.fp8 = prec.int8() ? 2 : 1;
        op.tw.wstream_e_frags = ti.e_frags;
        op.tw.wstream = im.upload(ti.w8);
    } else {
        op.tw.wstream = im.upload(ti.w);
    }
    op.tw.bstream = im.upload(ti.b);
    op.tw.pstream = im.upload(ti.p);
    op.tw.wstream_wave_frags = ti.w_wave_frags;
    op.tw.bstream_wave_floats = ti.b_wave_floats;
    op.tw.pstream_wave_bytes = ti.p_wave_bytes;
    op.tw.batch = B;
    op.tw.gate_in = tower_gate;
    if (dev.tower_trace) op.tw.trace = static_cast<unsigned long long*>(im.dalloc(2 * 256 * sizeof(unsigned long long)));
    prod_op = int(im.ops.size());
    im.ops.push_back(op);
    tower_blocks.clear();
    tower_gate = nullptr;
    std::swap(cur, nxt);
}

// the open float16x3 run: split-board launches (3x3 blocks of a small batch) or one tower launch
template <typename T> void RiseNet::Builder<T>::flush_x3_run() {
    if (x3_blocks.empty()) return;
    if (x3_split && x3_run_ks == 3) {
        if (!split_parts[0])
            for (auto& q : split_parts) q = static_cast<float*>(im.dalloc(size_t(B) * kSplitMaxG * kSquares * C * sizeof(float)));
        const int max_g = std::max(1, std::min(int(kSplitMaxG), net.cu_count_ / B));
        const int nb = int(x3_blocks.size());
        int gin = 1;
        for (int k = 0; k < nb; ++k) {
            Op op;
            op.kind = OpKind::BlockX3Split;
            op.xs.blk = x3_blocks[k];
            op.xs.x_parts = k == 0 ? reinterpret_cast<const float*>(cur) : split_parts[k % 2];
            op.xs.y_parts = split_parts[(k + 1) % 2];
            op.xs.gin = gin;
            op.xs.batch = B;
            op.xs.G = std::min(max_g, x3_blocks[k].cop_pad / block_x3_chunk_channels());
            op.xs.dev = dev.x3_split_dev;
            if (k > 0 && x3_blocks[k].se_kind != 0 && !(dev.x3_split_dev & 8)) {      // the launch before a gated block leaves its images' channel sums
                float* pools = static_cast<float*>(im.dalloc(size_t(B) * kSplitMaxG * C * sizeof(float)));
                im.ops.back().xs.pool_out = pools;
                op.xs.pool_in = pools;
            }
            gin = op.xs.G;
            im.ops.push_back(op);
        }
        Op fin;
        fin.kind = OpKind::X3SplitFinish;
        fin.xs.x_parts = split_parts[nb % 2];
        fin.xs.gin = gin;
        fin.xs.batch = B;
        fin.xs_y = reinterpret_cast<float*>(nxt);
        im.ops.push_back(fin);
    } else {
        Op op;
        op.kind = OpKind::TowerX3;
        op.tx.x = reinterpret_cast<const float*>(cur);
        op.tx.y = reinterpret_cast<float*>(nxt);
        op.tx.blocks = im.upload(x3_blocks);
        op.tx.nblocks = int(x3_blocks.size());
        op.tx.batch = B;
        op.tx.p8 = prec.p8() ? 1 : 0;
        op.tx.ks = x3_run_ks;
        op.tx.symmetric = dev.x3_symmetric ? 1 : 0;
        op.tx.no_tail = dev.x3_no_tail ? 1 : 0;
        op.tx.no_quad = dev.x3_no_quad ? 1 : 0;
        im.ops.push_back(op);
    }
    x3_blocks.clear();
    prod_op = -1;                      // these launches do not emit channel sums: a gate behind them is an SE launch of its own
    std::swap(cur, nxt);
}

template <typename T> void RiseNet::Builder<T>::one_launch_head() {
    // policy + value head in one launch (head.hip; stream layouts in kernels.h: HeadArgs)
    const Folded fv = fold_bn(nf, "value_head.body.0", "value_head.body.1");
    const HeadStreams hs = pack_head(fold_bn(nf, "policy_head.body.0", "policy_head.body.1"), fold_bn(nf, "policy_head.body.3", ""), fv, C, cv, cp);
    Op op;
    op.kind = OpKind::Head;
    HeadArgs& h = op.hd;
    h.x = cur;
    h.logits = net.d_logits_;
    h.probs = net.d_probs_;
    h.value = net.d_value_;
    h.aux = net.d_aux_;
    h.s1 = im.upload(hs.s1);
    h.b1 = im.upload(hs.b1);
    h.s2 = im.upload(hs.s2);
    h.s1_wave_frags = 9 * 16 + 16 + 16;
    h.s2_wave_frags = 18 * 3 + 9;
    h.vconv_bias = im.upload_d2f(fv.b, 8);
    h.cp = cp;
    h.batch = B;
    if (dev.tower_trace) h.trace = static_cast<unsigned long long*>(im.dalloc(64 * sizeof(unsigned long long)));
    const int nfl = kSquares * cv;
    if (wdl) {
        h.fc1_w = im.upload(pack_value_wdl(nf, nfl, 512));                 // [4][512], rows zero-padded beyond nfl
        const float* bw = nf.get("value_head.body_wdl.0.bias").data;
        h.wdl_b[0] = bw[0]; h.wdl_b[1] = bw[1]; h.wdl_b[2] = bw[2];
        h.wdl_b[3] = nf.get("value_head.body_plys.0.bias").data[0];
        h.wdlp = 1;
        macs += 4.0 * nfl;
    } else {
        const TensorView& w2 = nf.get("value_head.body_final.2.weight");
        const float* bb = nf.get("value_head.body_final.0.bias").data;
        h.fc1_w = im.upload(pack_value_fc1_threads(nf, nfl, fc));
        h.fc1_b = im.upload(std::vector<float>(bb, bb + fc));
        h.fc2_w = im.upload(std::vector<float>(w2.data, w2.data + fc));
        h.fc2_b = nf.get("value_head.body_final.2.bias").data[0];
        macs += double(nfl) * fc + fc;
    }
    macs += double(kSquares) * 9 * (double(C) * C + double(C) * cp) + double(kSquares) * C * cv;
    im.ops.push_back(op);
}

template <typename T> void RiseNet::Builder<T>::policy_head() {
    // _PolicyHead (select_policy_from_plane), builder_util.py:206-243
    // Precision float16p8, policy map at 256 channels: both convs of the head in ONE launch (x3.hip: conv3x3_p8_chain_kernel)
    // (a small batch: float16x3's convs, the first one's couts over four workgroups per board, the second beside the value head -- the
    // chain's 0.049 ms at batch 1 became 0.017 + 0.024, the latter shared with the value head: profiles/r06/f_*, y_*)
    const bool head_chain = prec.p8() && policy_map && C == 256 && round_up(cp, 16) <= 128 && !x3_split;
    // Precision float16x3 has the same head as one launch since round 6 (x3.hip: conv3x3_x3_chain_kernel, the same bits as the two launches);
    // CRA_X3_NO_HEAD_CHAIN: development A/B.  Small-batch nets keep the two launches (the first conv's couts over four workgroups per board).
    const bool head_chain_x3 = prec.x3() && !prec.p8() && prec.fused && policy_map && C == 256 && round_up(cp, 16) <= 128 && !x3_split &&
                               !dev.x3_no_head_chain;
    if (head_chain || head_chain_x3) {
        Folded f1 = fold_bn(nf, "policy_head.body.0", "policy_head.body.1");
        double inv1 = 1.0;
        SplitPack s1 = head_chain ? pack_dense_p8(f1, C, C, 3, C, C, &inv1) : pack_dense_split(f1, C, C, 3, C, C);
        add_conv("policy_head.body.3", "", cur, nullptr, nullptr, C, C, cp, 3, false, net.d_logits_, head_chain);   // (its x: the tower's output)
        ConvArgs& c = im.ops.back().conv;
        c.pre_wpk = im.upload(s1.hi);
        c.pre_wpk_lo = im.upload(s1.lo);
        c.pre_bias = im.upload_d2f(f1.b, C);
        c.pre_acc_scale = float(inv1);
        macs += double(kSquares) * C * C * 9;
        return;
    }
    // (a small batch: float16x3's convs in both modes, like its blocks -- the cross terms on e5m2 buy nothing where a launch is its latency)
    add_conv("policy_head.body.0", "policy_head.body.1", cur, nxt, nullptr, C, C, C, 3, true, nullptr, !x3_split);
    im.ops.back().conv.few_boards = x3_split ? dev.small_conv_split : 0;
    if (policy_map) {
        add_conv("policy_head.body.3", "", nxt, nullptr, nullptr, C, C, cp, 3, false, net.d_logits_, !x3_split);
        return;
    }
    // flat labels: conv3x3(C->P) + BN + ReLU written channel-major flat (x.view(-1, nb_flatten)), then Linear(P*64 -> n_labels)
    // as a GEMM over the BATCH (64 boards play the 64 "squares" of a workgroup tile), float logits row per board
    const int nfl = cp * kSquares, Bpad = round_up(B, 64);
    T* pflat = static_cast<T*>(im.dalloc(size_t(Bpad) * nfl * sizeof(T)));
    HIP_CHECK(hipMemset(pflat, 0, size_t(Bpad) * nfl * sizeof(T)));
    ConvArgs& c1 = conv_op(fold_bn(nf, "policy_head.body.3", "policy_head.body2.0"), nxt, pflat, C, C, cp, 3, 1);
    c1.out_flat = 1;
    c1.flat_pitch = nfl;
    macs += double(kSquares) * C * cp * 9;
    const TensorView& w = nf.get("policy_head.body3.0.weight");
    const float* bb = nf.get("policy_head.body3.0.bias").data;
    Folded fl;
    fl.w.assign(w.data, w.data + size_t(n_labels) * nfl);
    fl.b.assign(bb, bb + n_labels);
    ConvArgs& c2 = conv_op(fl, pflat, net.d_logits_, nfl, nfl, n_labels, 1, 0);
    c2.batch = Bpad / 64;
    c2.out_rows_f32 = 1;
    c2.rows_valid = B;
    macs += double(nfl) * n_labels;
}

// Precision float16x3, policy map: the policy conv holds a board's whole logit vector in one workgroup and runs the softmax itself
// (conv_gemm_x3_kernel; the launcher takes one workgroup per board up to 256 couts, the staging tiles hold 8192 logits); else a launch of its own
template <typename T> void RiseNet::Builder<T>::softmax() {
    if (prec.x3() && !im.ops.empty() && im.ops.back().kind == OpKind::Conv && im.ops.back().conv.out_policy_f32 &&
        im.ops.back().conv.cout_pad <= 256 && im.ops.back().conv.cout_real * kSquares <= 8192) {
        im.ops.back().fused_softmax = true;
    } else {
        Op op;
        op.kind = OpKind::Softmax;
        im.ops.push_back(op);
    }
}

template <typename T> void RiseNet::Builder<T>::value_head() {
    // CRA_X3_VALUE_HEAD=one / three: the float16x3 forward's value head as the one-launch f32 kernel or as the three launches below
    // (development: A/B and the lane determinism stress test, tests/test_lane_determinism_gpu.py)
    const bool x3_value_one_launch = prec.x3() && prec.fused && dev.x3_value_one_launch;
    const int nfl = kSquares * cv;
    if (prec.fused && !x3_value_one_launch) {
        // _ValueHead (builder_util.py:246-326) as three MFMA/wave-level launches instead of one latency-bound VALU kernel (Precision
        // float16 / fp8 layer paths; float16x3 on request).  Precision float16x3 runs the one-launch f32 kernel below (0.022 ms against
        // 0.039): in round 3 it made two-lane searches irreproducible -- its FC1 ran on v_pk_fma_f32, which goes wrong beside the MFMA
        // waves of the other lane's policy conv on the same SIMD (profiles/NOTES.md round 5); FC1 is on v_fmac_f32 since.
        //   (1) conv1x1(C->cv)+BN+ReLU on the conv-GEMM kernel, written channel-major flat  (x.view(-1, nb_flatten))
        //   (2) FC(nfl->fc)+ReLU as a GEMM over the BATCH: 64 boards play the role of the 64 "squares" of one workgroup tile
        //   (3) FC(fc->1)+tanh, or the WDLP outputs, one wave per board
        const int Bpad = round_up(B, 64);
        T* vflat = static_cast<T*>(im.dalloc(size_t(Bpad) * nfl * sizeof(T)));
        HIP_CHECK(hipMemset(vflat, 0, size_t(Bpad) * nfl * sizeof(T)));
        ConvArgs& c = conv_op(fold_bn(nf, "value_head.body.0", "value_head.body.1"), cur, vflat, C, C, cv, 1, 1);
        c.out_flat = 1;
        c.flat_pitch = nfl;
        macs += double(kSquares) * C * cv;
        Op fin;
        fin.kind = OpKind::ValueFinal;
        ValueFinalArgs& vf = fin.vf;
        vf.value = net.d_value_;
        vf.aux = net.d_aux_;
        vf.batch = B;
        if (wdl) {
            const float* bw = nf.get("value_head.body_wdl.0.bias").data;
            vf.in = vflat;
            vf.n = nfl;
            vf.w = im.upload(pack_value_wdl(nf, nfl, nfl));
            vf.b[0] = bw[0]; vf.b[1] = bw[1]; vf.b[2] = bw[2];
            vf.b[3] = nf.get("value_head.body_plys.0.bias").data[0];
            vf.wdlp = 1;
            macs += 4.0 * nfl;
        } else {
            if (nfl % 32 != 0) throw std::runtime_error("value head flatten size must be a multiple of 32");
            const TensorView &w1 = nf.get("value_head.body_final.0.weight"), &w2 = nf.get("value_head.body_final.2.weight");
            const float* b1 = nf.get("value_head.body_final.0.bias").data;
            Folded f1;
            f1.w.assign(w1.data, w1.data + size_t(fc) * nfl);
            f1.b.assign(b1, b1 + fc);
            const int fc_pad = round_up(fc, 16);
            T* vh = static_cast<T*>(im.dalloc(size_t(Bpad) * fc_pad * sizeof(T)));
            conv_op(f1, vflat, vh, nfl, nfl, fc, 1, 1).batch = Bpad / 64;        // 64 boards per workgroup tile
            vf.in = vh;
            vf.n = fc_pad;
            std::vector<float> w2p(fc_pad, 0.f);
            std::copy(w2.data, w2.data + fc, w2p.begin());
            vf.w = im.upload(w2p);
            vf.b[0] = nf.get("value_head.body_final.2.bias").data[0];
            vf.wdlp = 0;
            macs += double(nfl) * fc + fc;
        }
        im.ops.push_back(fin);
        return;
    }
    // _ValueHead, builder_util.py:246-326
    Folded fd = fold_bn(nf, "value_head.body.0", "value_head.body.1");
    Op op;
    op.kind = OpKind::ValueHead;
    ValueHeadArgs& v = op.vh;
    v.x = cur;
    v.wconv = im.upload_d2f(fd.w);
    v.bconv = im.upload_d2f(fd.b);
    v.value = net.d_value_;
    v.aux = net.d_aux_;
    v.batch = B;
    v.C = C;
    v.cv = cv;
    v.fc = fc;
    if (wdl) {
        const TensorView &ww = nf.get("value_head.body_wdl.0.weight"), &wp = nf.get("value_head.body_plys.0.weight");
        v.wwdl = im.upload(std::vector<float>(ww.data, ww.data + 3 * nfl));
        const float* bw = nf.get("value_head.body_wdl.0.bias").data;
        v.bwdl = im.upload(std::vector<float>(bw, bw + 3));
        v.wplys = im.upload(std::vector<float>(wp.data, wp.data + nfl));
        v.bplys = nf.get("value_head.body_plys.0.bias").data[0];
        macs += 4.0 * nfl;
    } else {
        const TensorView& w2 = nf.get("value_head.body_final.2.weight");
        v.w1t = im.upload(pack_value_fc1_transposed(nf, nfl, fc));
        const float* b1 = nf.get("value_head.body_final.0.bias").data;
        v.b1 = im.upload(std::vector<float>(b1, b1 + fc));
        v.w2 = im.upload(std::vector<float>(w2.data, w2.data + fc));
        v.b2 = nf.get("value_head.body_final.2.bias").data[0];
        macs += double(nfl) * fc + fc;
    }
    macs += double(kSquares) * C * cv;
    if (dev.value_head_debug) {                                     // development: stage checksums of every launch (ValueHeadArgs::dbg)
        // [B][8 + 1024] checksums and FC1 sums, then (variant & 16, the PROBE instantiation) [B][16 + 3 * 1024] words
        const size_t dbg_bytes = size_t(B) * ((8 + 1024) + (16 + 3 * 1024)) * sizeof(float);
        v.dbg = static_cast<float*>(im.dalloc(dbg_bytes));
        HIP_CHECK(hipMemset(v.dbg, 0, dbg_bytes));
        net.value_head_dbg_ = v.dbg;
    }
    v.lds_pad = dev.value_head_lds_pad;                            // default -1: no LDS fence (kernels.hip: round 5's root cause)
    v.variant = dev.value_head_variant;
    prepare_value_head<T>(op.vh);
    im.ops.push_back(op);
}

// a small batch: the policy conv that ends in the softmax and the value head side by side in one launch (x3.hip: heads_small_kernel);
// CRA_SMALL_BATCH_HEADS_APART: development A/B
template <typename T> void RiseNet::Builder<T>::merge_heads_small() {
    std::vector<Op>& ops = im.ops;
    if (x3_split && ops.size() >= 2 && ops.back().kind == OpKind::ValueHead && ops[ops.size() - 2].kind == OpKind::Conv &&
        ops[ops.size() - 2].fused_softmax && heads_small_fits(ops[ops.size() - 2].conv, ops.back().vh) && !dev.small_batch_heads_apart) {
        Op vh = ops.back();
        ops.pop_back();
        Op& op = ops.back();
        op.kind = OpKind::HeadsSmall;
        op.vh = vh.vh;
    }
}

// Precision float16x3, a net made for more than 64 boards: the policy chain's second conv has at most six cout tiles for eight waves, and
// the value head runs on the two idle ones (x3_heads.cpp: conv3x3_x3_heads_kernel, the bits of the two launches).  The op stays a Conv op
// with the chain's name; it carries the value head's arguments too.  Nets for at most 64 boards keep their heads (heads_small / value_head:
// the small-batch path and the co-residency screen work on those); CRA_X3_VALUE_HEAD / CRA_VALUE_HEAD_VARIANT ask for a value head kernel
// by name and get its launch; CRA_X3_HEADS_APART=1: the A/B reference.
template <typename T> void RiseNet::Builder<T>::merge_heads_x3() {
    std::vector<Op>& ops = im.ops;
    if (!(prec.x3() && !prec.p8() && B > RiseNet::kBoardSplitMaxBatch && !dev.x3_heads_apart && !dev.value_head_env && dev.conv_dev < 0)) return;
    if (ops.size() < 2 || ops.back().kind != OpKind::ValueHead || ops[ops.size() - 2].kind != OpKind::Conv) return;
    const Op& pol = ops[ops.size() - 2];
    if (!pol.fused_softmax || pol.from_planes || !heads_x3_fits(pol.conv, ops.back().vh) || pol.conv.batch != ops.back().vh.batch) return;
    const ValueHeadArgs vh = ops.back().vh;
    ops.pop_back();
    ops.back().heads_x3 = true;
    ops.back().vh = vh;
}

// stem -> tower -> head with nothing in between and nothing handed to other launches: one launch, the board tile stays in LDS
template <typename T> void RiseNet::Builder<T>::merge_forward() {
    std::vector<Op>& ops = im.ops;
    if (prec.one_launch && ops.size() == 3 && ops[0].kind == OpKind::Stem && ops[1].kind == OpKind::Tower && ops[2].kind == OpKind::Head &&
        ops[1].tw.gate_in == nullptr && ops[1].tw.pool_out == nullptr) {
        Op op;
        op.kind = OpKind::Forward;
        op.st = ops[0].st;
        op.tw = ops[1].tw;
        op.hd = ops[2].hd;
        ops.assign(1, op);
        init_forward_kernel_attributes();
    }
}

template <typename T> void RiseNet::build(const NetFile& nf) {
    Builder<T> b(*this, nf);
    b.read_model();
    b.stem();
    if (b.dense_blocks && b.tower_ok) b.dense_tower();
    else if (b.dense_blocks) b.dense_layer_blocks();
    else b.bottleneck_blocks();
    if (prec_.wnet && b.wblock_ops == 0 && b.wntb_ops == 0)
        throw std::runtime_error(std::string(prec_.wtower ? "`-wtower`" : "`-wnet`") + " runs the mobile-bottleneck and transformer blocks of 128 / 192 / 224-channel nets in one launch each: no block of this model qualifies (" +
                                 std::to_string(b.C) + " channels, " + (b.dense_blocks ? "dense residual blocks" : "mobile-bottleneck blocks") +
                                 "); use the precision without the suffix");
    if (prec_.wblock && !prec_.wnet && b.wblock_ops == 0)
        throw std::runtime_error("`-wblock` runs the mobile-bottleneck blocks of 128 / 192 / 224-channel nets in one launch each: no block of this model qualifies (" +
                                 std::to_string(b.C) + " channels, " + (b.dense_blocks ? "dense residual blocks" : "mobile-bottleneck blocks") +
                                 "); use the precision without the suffix");
    if (b.head_ok) {
        b.one_launch_head();
    } else {
        b.policy_head();
        b.softmax();
        b.value_head();
        b.merge_heads_small();
        b.merge_heads_x3();
    }
    init_block_kernel_attributes<T>();
    init_x3_kernel_attributes();
    init_x3_heads_kernel_attributes();
    init_x3_wblock_kernel_attributes();
    init_x3_wsplit_kernel_attributes();
    init_x3_wtower_kernel_attributes();
    init_x3_wntb_kernel_attributes();
    init_tower_kernel_attributes();
    init_restower_kernel_attributes();
    init_head_kernel_attributes();
    b.merge_forward();
    design_.flops_per_position = 2.0 * b.macs;
    launches_ = int(impl_->ops.size());
}

template void RiseNet::build<half_t>(const NetFile& nf);
template void RiseNet::build<float>(const NetFile& nf);

}  // namespace cra
