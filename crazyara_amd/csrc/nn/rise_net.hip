#include "rise_net.h"

#include <atomic>
#include <mutex>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <type_traits>
#include <stdexcept>
#include <algorithm>
#include <cctype>
#include <dirent.h>
#include <sys/stat.h>

#include "kernels.h"
#include "onnx_import.h"
#include "pack.h"
#include "../chess/planes_host.h"

namespace cra {

#define HIP_CHECK(expr)                                                                                      \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " #expr);      \
    } while (0)

namespace {
// the float16x3 forward's value head: false = conv GEMM + FC GEMM + value_final (three launches), true = value_head_kernel (one)
constexpr bool kX3ValueHeadOneLaunch = true;

enum class OpKind { PlanesToAct, Conv, Depthwise, SE, ValueHead, Softmax, Block, ValueFinal, SEGate, Tower, Head, Stem, ResTower, Forward, TowerX3, BlockX3Split, X3SplitFinish, HeadsSmall, Attention };

struct Op {
    OpKind kind;
    ConvArgs conv{};
    bool from_planes = false;     // float16x3 stem conv: reads the NCHW input planes (their address is a launch-time value too)
    bool fused_softmax = false;   // float16x3 policy-map conv: the softmax runs in its launch (the probabilities' address is a launch-time value)
    // depthwise / se
    const void* x = nullptr;
    void* y = nullptr;
    const float *w0 = nullptr, *w1 = nullptr, *b0 = nullptr;
    int C = 0, ks = 0, se_kind = 0;
    ValueHeadArgs vh{};
    BlockArgs blk{};
    ValueFinalArgs vf{};
    TowerArgs tw{};
    HeadArgs hd{};
    ResTowerArgs rt{};
    StemArgs st{};
    X3TowerArgs tx{};
    X3SplitArgs xs{};             // BlockX3Split; X3SplitFinish: x_parts, gin, batch and (xs_y) the float stream
    float* xs_y = nullptr;
};
}  // namespace

// development: what the co-residency screen knows about one op (RiseNet::dev_screen_prepare)
struct ScreenOp {
    struct Buf { char* live; char* before; char* after; size_t bytes; };
    std::vector<Buf> writes;          // the mutable buffers the op changes
    bool idempotent = true;           // launched again on its own result it gives the same bits
};

struct RiseNet::Impl {
    std::vector<void*> allocs;
    std::vector<std::pair<char*, size_t>> mutables;      // allocations that are not uploaded constants: activations, outputs, scratch
    std::vector<Op> ops;
    std::vector<ScreenOp> screen;
    std::vector<void*> screen_allocs;
    unsigned* screen_bad = nullptr;
    int cin_pad = 0;

    void* dalloc(size_t bytes, bool constant = false) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
        allocs.push_back(p);
        if (!constant) mutables.emplace_back(static_cast<char*>(p), bytes ? bytes : 16);
        return p;
    }
    template <typename U> U* upload(const std::vector<U>& h) {
        U* d = static_cast<U*>(dalloc(h.size() * sizeof(U), true));
        HIP_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice));
        return d;
    }
    float* upload_d2f(const std::vector<double>& h, size_t pad_to = 0) {
        std::vector<float> f(std::max(h.size(), pad_to), 0.f);
        for (size_t i = 0; i < h.size(); ++i) f[i] = float(h[i]);
        return upload(f);
    }
    ~Impl() {
        for (void* p : allocs) (void)hipFree(p);
        for (void* p : screen_allocs) (void)hipFree(p);
    }
};

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
    own_stream = getenv("CRA_OWN_STREAM_PER_NET") != nullptr;
    if (const char* e = getenv("CRA_SMALL_BATCH_CONV_SPLIT")) small_conv_split = atoi(e);
    tower_trace = getenv("CRA_TOWER_TRACE") != nullptr;
    x3_value_one_launch = kX3ValueHeadOneLaunch;
    if (const char* e = getenv("CRA_X3_VALUE_HEAD")) x3_value_one_launch = e[0] == 'o';
    value_head_debug = getenv("CRA_VALUE_HEAD_DEBUG") != nullptr;
    if (const char* e = getenv("CRA_VALUE_HEAD_LDS_PAD")) value_head_lds_pad = atoi(e);
    if (const char* e = getenv("CRA_VALUE_HEAD_VARIANT")) value_head_variant = atoi(e);
    x3_no_head_chain = getenv("CRA_X3_NO_HEAD_CHAIN") != nullptr;
    small_batch_heads_apart = getenv("CRA_SMALL_BATCH_HEADS_APART") != nullptr;
}

// The streams nets work in.  The runtime binds every stream to one of GPU_MAX_HW_QUEUES (4) hardware queues -- the one with the fewest
// streams on it, whether those streams do anything or not -- and two streams of one queue run strictly one after the other
// (scripts/ubench/stream_queues.hip, profiles/r06/v_stream_queues.txt: two 2 ms kernels take 4.0 ms on streams 0 and 7 of eight, 2.0 ms on
// any two of different queues).  With a stream created per net, which queue two evaluator lanes (or two NeuralNetAPIUsers) shared was
// decided by how many nets the process had opened before and not yet closed: the same two-lane search measured 35k or 63k nodes/s, the
// same two predict() users 302k or 359k evals/s, depending on nets that were idle at the time (profiles/r06/t_*, u_*).  So the library
// keeps one stream per hardware queue and device, made together on first need and never destroyed (their queues stay four different
// ones), and a new net takes the one that has gone unused the longest: idle nets do not keep a queue busy, and up to four nets that work
// at the same time work on four queues.  More nets than queues share streams as they shared queues before -- in order, which is correct
// for everything a net does (each net's work is in-order in its stream; graphs are captured on a stream of their own, see capture()).
namespace {
struct NetStreams {
    std::mutex mu;
    int n = 0;
    hipStream_t s[16] = {};
    std::atomic<uint64_t> last[16] = {};
};
NetStreams g_net_streams[64];                  // per device
std::atomic<uint64_t> g_stream_tick{1};

int take_net_stream(int device, hipStream_t* out) {
    NetStreams& ns = g_net_streams[device];
    std::lock_guard<std::mutex> lk(ns.mu);
    if (ns.n == 0) {
        int n = 4;                              // the runtime's default number of hardware queues per process and device
        if (const char* e = getenv("GPU_MAX_HW_QUEUES")) n = atoi(e);
        n = n < 1 ? 1 : n > 16 ? 16 : n;
        for (int i = 0; i < n; ++i) HIP_CHECK(hipStreamCreateWithFlags(&ns.s[i], hipStreamNonBlocking));
        ns.n = n;
    }
    int best = 0;
    for (int i = 1; i < ns.n; ++i)
        if (ns.last[i].load(std::memory_order_relaxed) < ns.last[best].load(std::memory_order_relaxed)) best = i;
    ns.last[best].store(g_stream_tick.fetch_add(1, std::memory_order_relaxed), std::memory_order_relaxed);
    *out = ns.s[best];
    return best;
}
}  // namespace

void RiseNet::touch_stream() const {
    if (stream_slot_ >= 0) g_net_streams[device_].last[stream_slot_].store(g_stream_tick.fetch_add(1, std::memory_order_relaxed), std::memory_order_relaxed);
}

static thread_local hipStream_t g_companion_stream = nullptr;   // set by a constructor for the constructor of its companion net (same thread, next statement)
static thread_local int g_companion_slot = -1;

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
            return v;
        }
    throw std::invalid_argument("unsupported precision '" + precision + "' (float16 | float16x3 | float16p8 | float32 | fp8 | int8)");
}

RiseNet::RiseNet(const std::string& model_path, int device_id, int batch_size, const std::string& precision)
    : device_(device_id), impl_(new Impl) {
    if (batch_size <= 0) throw std::invalid_argument("batch size must be positive");
    precision_arg_ = precision;
    prec_ = parse_precision(precision);
    design_.batch = batch_size;

    // model discovery (TensorrtAPI ctor, tensorrtapi.cpp:53-58)
    std::string dir, file;
    auto ends_with = [&](const char* ext) { const size_t n = strlen(ext); return model_path.size() > n && model_path.compare(model_path.size() - n, n, ext) == 0; };
    if (ends_with(".cranet") || ends_with(".onnx")) {
        const size_t sl = model_path.find_last_of('/');
        dir = sl == std::string::npos ? "./" : model_path.substr(0, sl + 1);
        file = sl == std::string::npos ? model_path : model_path.substr(sl + 1);
    } else {
        if (model_path.empty()) throw std::invalid_argument("The given directory must not be empty.");
        dir = model_path.back() == '/' ? model_path : model_path + "/";
        file = find_model_file(dir, batch_size);
    }
    model_name_ = file;
    model_file_path_ = dir + file;
    design_.version = read_version_from_string(model_name_);
    design_.game_phase = read_game_phase_from_string(dir);

    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) throw std::invalid_argument("device id out of range");
    HIP_CHECK(hipSetDevice(device_id));
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) cu_count_ = cus;
    }

    NetFile nf;                                  // load_model: our container, or the reference's ONNX parsed in place (onnx_import.h)
    if (model_file_path_.size() > 5 && model_file_path_.compare(model_file_path_.size() - 5, 5, ".onnx") == 0) import_onnx(model_file_path_, nf);
    else nf.load(model_file_path_);
    if (nf.str("arch") != "rise") throw std::runtime_error("unsupported arch '" + nf.str("arch") + "' in " + model_file_path_);
    if (g_companion_stream) {                    // the companion net of a larger one works in ITS stream (never at the same time: a call goes to one of them)
        stream_ = g_companion_stream;
        stream_slot_ = g_companion_slot;
        owns_stream_ = false;
        g_companion_stream = nullptr;
    } else if (dev_.own_stream || device_id >= 64) {
        HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    } else {
        stream_slot_ = take_net_stream(device_id, &stream_);
    }
    if (prec_.int8()) {
        int8_calib_ = read_int8_calibration(model_file_path_);
        if (int8_calib_.empty())
            throw std::runtime_error("Precision int8 needs a calibration of this model: " + int8_calibration_path(model_file_path_) +
                                     " is missing -- mi_net_calibrate_int8 makes it (integration/hipapi.h does that with the engine's calibration positions)");
    }
    if (prec_.fp16()) build<half_t>(nf); else build<float>(nf);   // init_nn_design + load_parameters + buffers
    capture();                                   // bind_executor
    // the companion net for calls with few boards (rise_net.h: small_) is made HERE, on the thread that makes this net: made on first use it
    // was made by whichever SearchThread came first, and two of them making nets at once -- one capturing its graph, one uploading weights
    // through the legacy stream -- is an error of the runtime ("would make the legacy stream depend on a capturing blocking stream")
    // It shares this net's stream: a stream of its own shifted which hardware queue every later stream of the process got, and two lanes
    // of a later search landed on ONE queue (config 1 with two lanes: 35k nodes/s instead of 63k, profiles/r06/t_*).
    if (!dev_.no_small_path && prec_.x3() && prec_.tower && prec_.fused && prec_.board_split && design_.batch > kBoardSplitMaxBatch) {
        g_companion_stream = stream_;
        g_companion_slot = stream_slot_;
        small_.reset(new RiseNet(model_file_path_, device_id, kBoardSplitMaxBatch, precision_arg_));
    }
}

static void turns_forget_stream(int device, hipStream_t s);     // below, next to RiseNet::Turn
// predict()s in flight per device (submit ... wait of any net): what decides between the two forms of a predict on pinned buffers (submit)
namespace {
std::atomic<int> g_predicts_in_flight[64];
}

RiseNet::~RiseNet() {
    if (counted_in_flight_) g_predicts_in_flight[device_].fetch_sub(1, std::memory_order_relaxed);
    (void)hipSetDevice(device_);
    small_.reset();                              // (it works in this net's stream)
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        if (owns_stream_ && stream_slot_ < 0) turns_forget_stream(device_, stream_);
    }
    experts_.clear();                            // (an expert set: every routed call was joined into stream_, drained above)
    if (route_) (void)hipHostFree(route_);
    if (fork_ev_) (void)hipEventDestroy(fork_ev_);
    for (hipEvent_t e : join_ev_) (void)hipEventDestroy(e);
    if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    impl_.reset();
    if (stream_ && owns_stream_ && stream_slot_ < 0) (void)hipStreamDestroy(stream_);
}

// ---- build(): the op list of the forward, stage by stage over one state (RiseNet::Builder) ----
namespace {
// which kernel family runs a bottleneck block (RiseNet::Builder::plan)
enum class Family {
    Tower,     // float16 / fp8 / int8: the one-launch tower (tower.hip), every block of the net in one run
    X3Tower,   // float16x3 / float16p8: a run of 3x3 or of 5x5 blocks in one launch (x3.hip: tower_x3_kernel, tower_p8_kernel)
    X3Split,   // float16x3 / float16p8 at small batches: a 3x3 block per launch over several workgroups per board (block_x3_split_kernel)
    Fused,     // one launch per block (kernels.hip: block_kernel; x3.hip: block_x3_kernel)
    Layers,    // expand, depthwise and project as three layer launches
    Transformer   // a NextViT transformer block: conv GEMMs and the attention kernel (Builder::transformer_block)
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
    double macs = 0;
    std::vector<TowerBlockDesc> tower_blocks;
    TowerStreams tower_streams;
    const float* tower_gate = nullptr;
    std::vector<X3TowerBlock> x3_blocks;
    int x3_run_ks = 3;                // a run is all 3x3 or all 5x5 blocks (tower_x3_roles_kernel<KS>, tower_p8_kernel<KS>)
    float* split_parts[2] = {nullptr, nullptr};
    static constexpr int kSplitMaxG = 10;

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
    void flush_tower();
    void flush_x3_run();
    void one_launch_head();
    void policy_head();
    void softmax();
    void value_head();
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
    if (ntb[i]) return {Family::Transformer, false};
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
        if (bp.family == Family::Transformer) {
            transformer_block(i);
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
            add_se(se_op(se), bp.family == Family::Fused);
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
    if (b.head_ok) {
        b.one_launch_head();
    } else {
        b.policy_head();
        b.softmax();
        b.value_head();
        b.merge_heads_small();
    }
    init_block_kernel_attributes<T>();
    init_x3_kernel_attributes();
    init_tower_kernel_attributes();
    init_restower_kernel_attributes();
    init_head_kernel_attributes();
    b.merge_forward();
    design_.flops_per_position = 2.0 * b.macs;
    launches_ = int(impl_->ops.size());
}

template <typename T> void RiseNet::launch_op(int i, hipStream_t s, const IoOverride* io) {
    Impl& im = *impl_;
    const int B = dyn_n_ > 0 ? dyn_n_ : design_.batch;       // (a forward of fewer boards than the net was made for: small_net())
    const Op& op = im.ops[i];
    auto boards = [&](ConvArgs c) {                            // a board-batched conv of such a forward
        if (dyn_n_ > 0 && c.batch == design_.batch && !c.out_rows_f32) c.batch = dyn_n_;
        return c;
    };
    // io: the caller's pinned host buffers stand in for the device-side input / output tensors of this forward (zero-copy predict)
    const float* planes = io ? io->planes : d_planes_;
    float* value = io ? io->value : d_value_;
    float* probs = io ? io->probs : d_probs_;
    float* aux = (io && d_aux_) ? (io->aux ? io->aux : d_aux_) : d_aux_;
    switch (op.kind) {
        case OpKind::PlanesToAct:
            launch_planes_to_act<T>(op.x == d_planes_ ? planes : static_cast<const float*>(op.x), static_cast<T*>(op.y), B, op.C, im.cin_pad, s);
            break;
        case OpKind::Conv:
            if (prec_.x3() && dev_.conv_dev >= 0) {                                // development: bisecting switches of conv_gemm_x3_kernel
                ConvArgs c = boards(op.conv);
                c.dev = dev_.conv_dev;
                if (op.from_planes) c.planes = planes;
                if (op.fused_softmax) { c.softmax_out = probs; if (!keep_logits_) c.out = nullptr; }
                launch_conv_gemm_x3(c, s);
            } else if (prec_.x3() && op.from_planes) {
                ConvArgs c = boards(op.conv);
                c.planes = planes;
                launch_conv_gemm_x3(c, s);
            } else if (prec_.x3() && op.fused_softmax) {
                ConvArgs c = boards(op.conv);
                c.softmax_out = probs;
                if (!keep_logits_) c.out = nullptr;          // (the logits stay in LDS unless a test / analysis asked for them)
                launch_conv_gemm_x3(c, s);
            } else if (prec_.x3()) launch_conv_gemm_x3(boards(op.conv), s);
            else launch_conv_gemm<T>(op.conv, s);
            break;
        case OpKind::Depthwise:
            launch_depthwise<T>(static_cast<const T*>(op.x), static_cast<T*>(op.y), op.w0, op.b0, B, op.C, op.ks, s);
            break;
        case OpKind::SE: launch_se<T>(static_cast<T*>(op.y), op.se_kind, op.w0, op.w1, op.b0, B, op.C, s, static_cast<const T*>(op.x)); break;
        case OpKind::ValueHead: {
            ValueHeadArgs v = op.vh;
            v.value = value;
            v.aux = aux;
            if (dyn_n_ > 0) v.batch = dyn_n_;
            launch_value_head<T>(v, s);
            break;
        }
        case OpKind::HeadsSmall: {
            HeadsSmallArgs h;
            h.conv = boards(op.conv);
            h.conv.softmax_out = probs;
            if (!keep_logits_) h.conv.out = nullptr;
            h.vh = op.vh;
            h.vh.value = value;
            h.vh.aux = aux;
            h.vh.batch = h.conv.batch;
            launch_heads_small(h, s);
            break;
        }
        case OpKind::Softmax: launch_softmax(d_logits_, probs, B, design_.nb_policy, s); break;
        case OpKind::Block:
            if (prec_.x3()) launch_block_x3(op.blk, s);
            else launch_block<T>(op.blk, s);
            break;
        case OpKind::ValueFinal: {
            ValueFinalArgs v = op.vf;
            v.value = value;
            v.aux = aux;
            launch_value_final<T>(v, s);
            break;
        }
        case OpKind::Tower: launch_tower(op.tw, s); break;
        case OpKind::Head: {
            HeadArgs h = op.hd;
            h.value = value;
            h.probs = probs;
            h.aux = aux;
            h.logits = keep_logits_ ? d_logits_ : nullptr;
            launch_head(h, s);
            break;
        }
        case OpKind::ResTower: launch_restower(op.rt, s); break;
        case OpKind::TowerX3:
            if (dyn_n_ > 0) {
                X3TowerArgs t = op.tx;
                t.batch = dyn_n_;
                launch_tower_x3(t, s);
            } else launch_tower_x3(op.tx, s);
            break;
        case OpKind::BlockX3Split:
            if (dyn_n_ > 0) {                                    // the workgroups per board follow the boards of THIS forward; a launch reads
                X3SplitArgs a = op.xs;                           // as many images per board as the launch before it wrote
                a.batch = dyn_n_;
                a.G = std::max(1, std::min(std::min(10, cu_count_ / dyn_n_), a.blk.cop_pad / block_x3_chunk_channels()));
                a.gin = (i == 0 || im.ops[i - 1].kind != OpKind::BlockX3Split) ? 1 : dyn_prev_g_;      // (a run's first block reads the float stream)
                dyn_prev_g_ = a.G;
                launch_block_x3_split(a, s);
            } else launch_block_x3_split(op.xs, s);
            break;
        case OpKind::X3SplitFinish: launch_x3_split_finish(op.xs.x_parts, dyn_n_ > 0 ? dyn_prev_g_ : op.xs.gin, op.xs_y, B, s); break;
        case OpKind::Stem: {
            StemArgs st = op.st;
            st.planes = planes;
            launch_stem(st, s);
            break;
        }
        case OpKind::Forward: {
            StemArgs st = op.st;
            HeadArgs h = op.hd;
            st.planes = planes;
            h.value = value;
            h.probs = probs;
            h.aux = aux;
            h.logits = keep_logits_ ? d_logits_ : nullptr;
            launch_forward(st, op.tw, h, s);
            break;
        }
        case OpKind::Attention: {
            AttentionArgs at{op.x, op.y, B, op.C, prec_.fp16() ? 0 : prec_.x3() ? 2 : 1};
            launch_attention(at, s);
            break;
        }
        case OpKind::SEGate:
            launch_se_gate(static_cast<const float*>(op.x), static_cast<float*>(op.y), op.se_kind, op.w0, op.w1, op.b0, B, op.C, s);
            break;
    }
}

template <typename T> void RiseNet::enqueue(hipStream_t s, const IoOverride* io) {
    // (Round 6 tried the value head of a small batch on a side stream beside the policy head -- two branches of the captured graph: the
    // forward got SLOWER, 0.354 against 0.335 ms at batch 1, the cross-queue joins cost more than the 24 us they hide: profiles/r06/e_*.)
    dyn_prev_g_ = 1;
    for (int i = 0; i < int(impl_->ops.size()); ++i) launch_op<T>(i, s, io);
    HIP_CHECK(hipGetLastError());
}

const char* RiseNet::op_name(int i) const {
    const Op& op = impl_->ops.at(i);
    switch (op.kind) {
        case OpKind::PlanesToAct: return "planes_to_act";
        case OpKind::Conv: return prec_.x3() ? (op.conv.ks == 1 ? "conv_gemm_x3_1x1" : "conv_gemm_x3_3x3") : (op.conv.ks == 1 ? "conv_gemm_1x1" : "conv_gemm_3x3");
        case OpKind::Depthwise: return "depthwise";
        case OpKind::SE: return "se";
        case OpKind::ValueHead: return "value_head";
        case OpKind::Softmax: return "softmax";
        case OpKind::Block: return prec_.x3() ? "block_x3" : "fused_block";
        case OpKind::ValueFinal: return "value_final";
        case OpKind::SEGate: return "se_gate";
        case OpKind::Tower: return "tower";
        case OpKind::Head: return "head";
        case OpKind::ResTower: return "restower";
        case OpKind::Stem: return "stem";
        case OpKind::Forward: return "forward";
        case OpKind::TowerX3: return op.tx.p8 ? "tower_p8" : "tower_x3";
        case OpKind::BlockX3Split: return "block_x3_split";
        case OpKind::X3SplitFinish: return "x3_split_finish";
        case OpKind::HeadsSmall: return "heads_small";
        case OpKind::Attention: return "attention";
    }
    return "?";
}

void RiseNet::time_ops(int iters, float* ms) {
    refuse_on_expert_set("per-op timing");
    HIP_CHECK(hipSetDevice(device_));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    const int n = int(impl_->ops.size());
    for (int it = 0; it < iters; ++it)
        for (int i = 0; i < n; ++i) {
            HIP_CHECK(hipEventRecord(e0, stream_));
            if (prec_.fp16()) launch_op<half_t>(i, stream_); else launch_op<float>(i, stream_);
            HIP_CHECK(hipEventRecord(e1, stream_));
            HIP_CHECK(hipEventSynchronize(e1));
            float t = 0.f;
            HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
            ms[i] += t;
        }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    for (const Op& op : impl_->ops)
        if ((op.kind == OpKind::Head || op.kind == OpKind::Forward) && op.hd.trace) {
            unsigned long long h[16];
            HIP_CHECK(hipMemcpy(h, op.hd.trace, sizeof(h), hipMemcpyDeviceToHost));
            fprintf(stderr, "head trace (load, conv1, pack, conv2, atomics, softmax, value):");
            for (int i = 1; i < 8; ++i) fprintf(stderr, " %llu", h[i] - h[i - 1]);
            fprintf(stderr, "\n");
        }
    for (const Op& op : impl_->ops)
        if ((op.kind == OpKind::Tower || op.kind == OpKind::Forward) && op.tw.trace) {
            std::vector<unsigned long long> h(512);
            HIP_CHECK(hipMemcpy(h.data(), op.tw.trace, 512 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (int wv = 0; wv < 2; ++wv) {
                fprintf(stderr, "tower trace wave %d:", wv * 4);
                for (int i = 1; i < 256 && h[wv * 256 + i]; ++i) fprintf(stderr, " %llu", h[wv * 256 + i] - h[wv * 256 + i - 1]);
                fprintf(stderr, "\n");
            }
        }
}

// ---- development: the co-residency screen ----
namespace {
// 16-byte pieces of two buffers compared in place; every differing piece counts into *bad (one word per launch of the screened op)
__global__ __launch_bounds__(256) void screen_compare_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, size_t n16, unsigned* bad) {
    unsigned diff = 0;
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < n16; i += size_t(gridDim.x) * 256) {
        const uint4 x = a[i], y = b[i];
        diff += (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) ? 1u : 0u;
    }
    if (diff) atomicAdd(bad, diff);
}
void screen_compare(const char* a, const char* b, size_t bytes, unsigned* bad, hipStream_t s) {
    const size_t n16 = bytes / 16;                       // (allocations are multiples of 16 bytes or compared up to the last whole piece)
    if (!n16) return;
    const int blocks = int(std::min<size_t>(512, (n16 + 255) / 256));
    hipLaunchKernelGGL(screen_compare_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const uint4*>(a), reinterpret_cast<const uint4*>(b), n16, bad);
}
}  // namespace

int RiseNet::dev_screen_prepare() {
    refuse_on_expert_set("the co-residency screen");
    HIP_CHECK(hipSetDevice(device_));
    Impl& im = *impl_;
    if (!im.screen.empty()) return int(im.screen.size());
    auto salloc = [&](size_t bytes) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
        im.screen_allocs.push_back(p);
        return static_cast<char*>(p);
    };
    im.screen_bad = reinterpret_cast<unsigned*>(salloc(sizeof(unsigned) * 65536));
    unsigned* flag = reinterpret_cast<unsigned*>(salloc(sizeof(unsigned) * im.mutables.size()));
    std::vector<char*> snap(im.mutables.size());
    for (size_t i = 0; i < im.mutables.size(); ++i) snap[i] = salloc(im.mutables[i].second);
    HIP_CHECK(hipStreamSynchronize(stream_));
    im.screen.resize(im.ops.size());
    std::vector<unsigned> hflag(im.mutables.size());
    for (int k = 0; k < int(im.ops.size()); ++k) {
        for (size_t i = 0; i < im.mutables.size(); ++i)
            HIP_CHECK(hipMemcpyAsync(snap[i], im.mutables[i].first, im.mutables[i].second, hipMemcpyDeviceToDevice, stream_));
        HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(unsigned) * im.mutables.size(), stream_));
        dev_launch_op(k, 1);
        for (size_t i = 0; i < im.mutables.size(); ++i) screen_compare(snap[i], im.mutables[i].first, im.mutables[i].second, flag + i, stream_);
        HIP_CHECK(hipMemcpyAsync(hflag.data(), flag, sizeof(unsigned) * hflag.size(), hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
        ScreenOp& so = im.screen[k];
        for (size_t i = 0; i < im.mutables.size(); ++i) {
            if (!hflag[i]) continue;
            ScreenOp::Buf b{im.mutables[i].first, salloc(im.mutables[i].second), salloc(im.mutables[i].second), im.mutables[i].second};
            HIP_CHECK(hipMemcpyAsync(b.before, snap[i], b.bytes, hipMemcpyDeviceToDevice, stream_));
            HIP_CHECK(hipMemcpyAsync(b.after, b.live, b.bytes, hipMemcpyDeviceToDevice, stream_));
            so.writes.push_back(b);
        }
        // the op once more, on its own result
        HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(unsigned), stream_));
        dev_launch_op(k, 1);
        for (const ScreenOp::Buf& b : so.writes) screen_compare(b.after, b.live, b.bytes, flag, stream_);
        HIP_CHECK(hipMemcpyAsync(hflag.data(), flag, sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
        so.idempotent = hflag[0] == 0;
        if (!so.idempotent)                                   // leave the forward's state behind the op as it was
            for (const ScreenOp::Buf& b : so.writes) HIP_CHECK(hipMemcpyAsync(b.live, b.after, b.bytes, hipMemcpyDeviceToDevice, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
    return int(im.screen.size());
}

long RiseNet::dev_screen_run(int op, int launches, long* words) {
    refuse_on_expert_set("the co-residency screen");
    HIP_CHECK(hipSetDevice(device_));
    Impl& im = *impl_;
    if (im.screen.empty()) throw std::runtime_error("dev_screen_run: dev_screen_prepare first");
    if (op < 0 || op >= int(im.screen.size())) throw std::invalid_argument("op index out of range");
    launches = std::min(launches, 65536);
    const ScreenOp& so = im.screen[op];
    HIP_CHECK(hipMemsetAsync(im.screen_bad, 0, sizeof(unsigned) * launches, stream_));
    for (int l = 0; l < launches; ++l) {
        if (!so.idempotent)
            for (const ScreenOp::Buf& b : so.writes) HIP_CHECK(hipMemcpyAsync(b.live, b.before, b.bytes, hipMemcpyDeviceToDevice, stream_));
        dev_launch_op(op, 1);
        for (const ScreenOp::Buf& b : so.writes) screen_compare(b.after, b.live, b.bytes, im.screen_bad + l, stream_);
        if ((l & 63) == 63) HIP_CHECK(hipStreamSynchronize(stream_));      // (keeps the queue short; the neighbour's stream runs on)
    }
    std::vector<unsigned> bad(launches);
    HIP_CHECK(hipMemcpyAsync(bad.data(), im.screen_bad, sizeof(unsigned) * launches, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    long n = 0, w = 0;
    for (unsigned b : bad) { n += b != 0; w += b; }
    if (words) *words = w;
    return n;
}

std::string RiseNet::dev_screen_info(int op) const {
    refuse_on_expert_set("the co-residency screen");
    const Impl& im = *impl_;
    if (op < 0 || op >= int(im.screen.size())) return "";
    size_t bytes = 0;
    for (const ScreenOp::Buf& b : im.screen[op].writes) bytes += b.bytes;
    return std::string(op_name(op)) + " writes " + std::to_string(im.screen[op].writes.size()) + " buffers / " + std::to_string(bytes) + " bytes" +
           (im.screen[op].idempotent ? "" : ", not idempotent (buffers restored before every launch)");
}

void RiseNet::dev_launch_op(int op, int iters) {
    refuse_on_expert_set("a single op");
    HIP_CHECK(hipSetDevice(device_));
    if (op < 0 || op >= int(impl_->ops.size())) throw std::invalid_argument("op index out of range");
    for (int it = 0; it < iters; ++it) {
        if (prec_.fp16()) launch_op<half_t>(op, stream_); else launch_op<float>(op, stream_);
    }
    HIP_CHECK(hipGetLastError());
}

float RiseNet::time_forward(int iters) {
    refuse_on_expert_set("a device-resident forward");
    HIP_CHECK(hipSetDevice(device_));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, stream_));
    for (int it = 0; it < iters; ++it) HIP_CHECK(hipGraphLaunch(graph_exec_, stream_));
    HIP_CHECK(hipEventRecord(e1, stream_));
    HIP_CHECK(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return t;
}

void RiseNet::keep_logits(bool on) {
    if (on == keep_logits_) return;
    keep_logits_ = on;
    for (auto& e : experts_) {                // an expert set: its experts (and their companions) keep them, the set collects the rows
        e->keep_logits(on);
        if (e->small_) e->small_->keep_logits(on);
    }
    if (launches_ > 1 && graph_exec_) {      // forwards of several launches replay a captured graph: capture again with the new head arguments
        HIP_CHECK(hipStreamSynchronize(stream_));
        (void)hipGraphExecDestroy(graph_exec_);
        if (graph_) (void)hipGraphDestroy(graph_);
        graph_exec_ = nullptr;
        graph_ = nullptr;
        capture();
    }
}

void RiseNet::capture() {
    // on a stream of its own: stream_ may be shared with a net that another thread is working with right now (NetStreams), and whatever
    // that thread launched between Begin and End would land in THIS graph
    hipStream_t cs = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipError_t err = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (err != hipSuccess) {
        (void)hipStreamDestroy(cs);
        HIP_CHECK(err);
    }
    try {
        forward_on(cs);
    } catch (...) {
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(cs, &g);
        if (g) (void)hipGraphDestroy(g);
        (void)hipStreamDestroy(cs);
        throw;
    }
    err = hipStreamEndCapture(cs, &graph_);
    (void)hipStreamDestroy(cs);
    HIP_CHECK(err);
    HIP_CHECK(hipGraphInstantiate(&graph_exec_, graph_, nullptr, nullptr, 0));
}

void RiseNet::forward_on(hipStream_t s) {
    refuse_on_expert_set("a forward without boards");
    if (prec_.fp16()) enqueue<half_t>(s); else enqueue<float>(s);
}

// Forwards of DIFFERENT streams take turns when a forward fills the chip on its own (one workgroup per board, 160 KiB of LDS: one
// per CU).  Two evaluator lanes (or two NeuralNetAPIUsers) keep two batches in flight on two streams; when the streams sit on
// different hardware queues the dispatcher interleaves the workgroups of both forward kernels, both batches then finish together after
// 2 x 0.31 ms, the host collects for both lanes with nothing queued, and the chip idles for every collect: measured 0.42 ms per batch
// instead of 0.32 on the headline search leg (615k against 750k nodes/s), in one mode or the other for a whole process depending
// on which queues the runtime handed out.  Taking turns (submission order) keeps one batch executing and one queued.  Small batches
// are left alone: a batch of 8 occupies 8 CUs and SHOULD overlap with its neighbour.  The copy path of predict() gains too (its D2H copies
// now run beside the other user's forward: two users 559k -> 767k evals/s); zero-copy predict is exempt (see submit()).
namespace {
struct ForwardTurns {
    std::mutex mu;
    hipEvent_t ev[64];
    bool made = false, any = false;
    bool multi = false;                   // a second stream has shown up: from then on every forward records its event
    int last = 0;
    hipStream_t last_stream = nullptr;
};
ForwardTurns g_turns[64];     // per device
}  // namespace

static void turns_forget_stream(int device, hipStream_t s) {    // the stream is about to be destroyed (and has been drained)
    if (device < 0 || device >= 64) return;
    std::lock_guard<std::mutex> lk(g_turns[device].mu);
    if (g_turns[device].last_stream == s) {
        g_turns[device].last_stream = nullptr;
        g_turns[device].any = false;
    }
}

struct RiseNet::Turn {
    ForwardTurns* t = nullptr;
    hipStream_t s = nullptr;
    std::unique_lock<std::mutex> lk;       // a member: released also when the constructor throws
    Turn(RiseNet& n) {
        static const bool off = getenv("CRA_NO_FORWARD_TURNS") != nullptr;      // development: A/B
        static const bool always = getenv("CRA_FORCE_FORWARD_TURNS") != nullptr;
        if (off || n.device_ < 0 || n.device_ >= 64 || (!always && int(n.design_.batch) * 4 < n.cu_count_ * 3)) return;
        ForwardTurns* ft = &g_turns[n.device_];
        lk = std::unique_lock<std::mutex>(ft->mu);
        if (!ft->made) {
            HIP_CHECK(hipSetDevice(n.device_));
            for (hipEvent_t& e : ft->ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ft->made = true;
        }
        if (!ft->multi) {
            // one stream on this device so far (a device-resident loop over one net: the headline measurement): nothing to order, and
            // an event record per forward is not free (measured 3 us per 0.33 ms step)
            if (ft->last_stream == nullptr || ft->last_stream == n.stream_) {
                ft->last_stream = n.stream_;
                lk.unlock();
                return;
            }
            // a second stream: everything the first one has been given so far goes in front of this forward
            ft->multi = true;
            if (hipEventRecord(ft->ev[0], ft->last_stream) == hipSuccess) {
                ft->last = 0;
                ft->any = true;
            } else {
                (void)hipGetLastError();          // that stream is gone (its net was closed): nothing of it can be in flight
            }
        }
        if (ft->any && ft->last_stream != n.stream_) HIP_CHECK(hipStreamWaitEvent(n.stream_, ft->ev[ft->last], 0));
        t = ft;
        s = n.stream_;
    }
    ~Turn() {
        if (!t) return;
        const int next = (t->last + 1) & 63;
        if (hipEventRecord(t->ev[next], s) == hipSuccess) {
            t->last = next;
            t->last_stream = s;
            t->any = true;
        }
    }
};

// Device-resident replay.  A forward that is ONE kernel gains nothing from a graph (there is no launch sequence to save) and loses the
// graph launch's own cost between consecutive replays: it goes into the stream as a plain launch.  Everything else replays the graph.
// CRA_DEVICE_GRAPH=1 forces the graph (A/B timing).
void RiseNet::forward_async() {
    refuse_on_expert_set("a device-resident forward");
    touch_stream();
    Turn turn(*this);
    if (launches_ == 1 && !dev_.device_graph) {
        forward_on(stream_);
        HIP_CHECK(hipGetLastError());
        return;
    }
    HIP_CHECK(hipGraphLaunch(graph_exec_, stream_));
}

// The forward between other work of the same stream (descriptor expansion before, gather / copies after).  A graph launch runs its
// nodes on the graph's own queue and is tied to the launching stream by cross-queue dependencies, which this runtime resolves from
// the host: measured, a lane's next kernel did not start until the host called into the runtime again (0.09-0.15 ms per batch lost
// whenever the host was busy collecting).  With the whole forward in one to five kernels there is nothing left for a graph to save,
// so these paths put the kernels straight into the stream: one queue, in-order, no host in the loop (float16p8's five launches: config 2
// searched at 373k nodes/s against 370k through the graph on an idle host, profiles/r04/ac_*).
void RiseNet::launch_forward_in_stream() {
    touch_stream();
    Turn turn(*this);
    if (dyn_n_ > 0 || (launches_ <= 5 && !dev_.lane_graph) || dev_.lane_no_graph) forward_on(stream_);      // (a forward of fewer boards: its own arguments)
    else HIP_CHECK(hipGraphLaunch(graph_exec_, stream_));
}

// every buffer of the call in pinned (device-visible) host memory?  Asked of the runtime on EVERY call (hipPointerGetAttributes: a
// microsecond or two per pointer against a forward of 100+ us): a remembered answer would outlive a hipHostFree / hipHostUnregister of
// the caller's buffers, and a later call with pageable memory at the same addresses would then be read and written by the kernels.
bool RiseNet::buffers_are_pinned(const float* in_planes, float* value, float* probs, float* aux) {
    if (dev_.predict_copy) return false;     // (CRA_PREDICT_COPY when the net was made: bench.py times the copy path on nets of its own)
    const void* set[4] = {in_planes, value, probs, (d_aux_ && aux) ? aux : nullptr};
    for (const void* p : set) {
        if (!p) continue;
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;     // the kernels read / write the buffers in 16-byte units
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess) {
            (void)hipGetLastError();               // a pageable pointer is reported as an error by some runtimes: not ours to keep
            return false;
        }
        if (at.type != hipMemoryTypeHost) return false;
    }
    return true;
}

void RiseNet::submit(const float* in_planes, float* value, float* probs, float* aux) {
    refuse_on_expert_set("predict / submit", "float planes carry no game phase -- mi_net_predict_routed takes the phases from the caller, mi_net_submit_boards derives them from the descriptors");
    HIP_CHECK(hipSetDevice(device_));   // every predict selects its device, tensorrtapi.cpp:198
    const size_t B = design_.batch;
    // Zero-copy or staged?  With pinned buffers the kernels can read the planes and write value / probabilities across PCIe themselves: no
    // copy commands, the best form for ONE user (338k against 331k evals/s at batch 256, profiles/r05/p_*).  With a second user's forward
    // on the device the staged form wins by 6 - 12 % in every measurement (422k against 377k: the copies of one user run on the DMA
    // engines beside the other user's forward, while a zero-copy forward holds its CUs for the whole PCIe write): so the form is chosen
    // from what is in flight when the call arrives -- the reference's default is Threads = 2 (optionsuci.cpp), i.e. two users.
    // CRA_PREDICT_COPY / CRA_PREDICT_ZERO_COPY (when the net was made) force one form.
    const bool others_in_flight = device_ >= 0 && device_ < 64 && g_predicts_in_flight[device_].load(std::memory_order_relaxed) > (counted_in_flight_ ? 1 : 0);
    if (!counted_in_flight_ && device_ >= 0 && device_ < 64) {
        g_predicts_in_flight[device_].fetch_add(1, std::memory_order_relaxed);
        counted_in_flight_ = true;
    }
    // with hysteresis: a user that has met another one in flight stays on the staged form for its next 64 calls (two blocking users drift in
    // and out of phase: one of them would otherwise find the device "empty" at every other call and alternate between the forms)
    if (others_in_flight) staged_calls_left_ = 64;
    else if (staged_calls_left_ > 0) --staged_calls_left_;
    last_zero_copy_ = buffers_are_pinned(in_planes, value, probs, aux) && (dev_.predict_zero_copy || staged_calls_left_ == 0);
    if (last_zero_copy_) {
        IoOverride io;
        io.planes = in_planes;
        io.value = value;
        io.probs = probs;
        io.aux = (d_aux_ && aux) ? aux : nullptr;
        // no turn-taking here: these kernels write 5 MB of probabilities per batch across PCIe from inside the forward, and two users
        // in flight hide each other's write phase only when their kernels interleave (measured: 770k against 585k evals/s)
        if (prec_.fp16()) enqueue<half_t>(stream_, &io); else enqueue<float>(stream_, &io);
        return;
    }
    HIP_CHECK(hipMemcpyAsync(d_planes_, in_planes, B * design_.nb_input_channels * kSquares * sizeof(float), hipMemcpyHostToDevice, stream_));
    launch_forward_in_stream();
    HIP_CHECK(hipMemcpyAsync(value, d_value_, B * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(probs, d_probs_, B * design_.nb_policy * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (d_aux_ && aux) HIP_CHECK(hipMemcpyAsync(aux, d_aux_, B * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
}

// a float16x3 / float16p8 net made for more than kBoardSplitMaxBatch boards, asked for at most that many: the companion net's business
bool RiseNet::small_path_ok() const {
    return small_ != nullptr;
}
RiseNet& RiseNet::small_net() { return *small_; }

void RiseNet::submit_boards(const void* descs_host, int n_valid, int layout, float* value, float* probs, float* aux, int routing) {
    HIP_CHECK(hipSetDevice(device_));
    const size_t B = design_.batch;
    if (n_valid < 0 || size_t(n_valid) > B) throw std::invalid_argument("n_valid out of range");
    if (layout_channels(layout) != design_.nb_input_channels)
        throw std::invalid_argument("plane layout has " + std::to_string(layout_channels(layout)) + " channels, net expects " +
                                    std::to_string(design_.nb_input_channels));
    if (!experts_.empty()) {
        submit_boards_routed(descs_host, n_valid, layout, value, probs, aux, routing);
        return;
    }
    if (n_valid > 0 && n_valid <= kBoardSplitMaxBatch && small_path_ok()) {
        small_net().submit_boards(descs_host, n_valid, layout, value, probs, aux);      // (into this net's stream: wait() as ever)
        return;
    }
    // (this net as the companion of a larger one: a forward of n_valid boards, and only their results go back)
    const bool partial = n_valid > 0 && prec_.x3() && prec_.board_split && design_.batch <= kBoardSplitMaxBatch && size_t(n_valid) < B && !dev_.no_small_path;
    const size_t rows = partial ? size_t(n_valid) : B;
    if (n_valid > 0) {
        HIP_CHECK(hipMemcpyAsync(d_desc_, descs_host, size_t(n_valid) * sizeof(BoardDesc), hipMemcpyHostToDevice, stream_));
        launch_planes_from_desc(static_cast<const BoardDesc*>(d_desc_), n_valid, layout, 1, d_planes_, stream_);
    }
    dyn_n_ = partial ? n_valid : 0;
    launch_forward_in_stream();
    dyn_n_ = 0;
    HIP_CHECK(hipMemcpyAsync(value, d_value_, rows * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(probs, d_probs_, rows * design_.nb_policy * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (d_aux_ && aux) HIP_CHECK(hipMemcpyAsync(aux, d_aux_, rows * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
}

void RiseNet::submit_boards_gathered(const void* descs_host, int n_valid, int layout, const uint16_t* idx, const uint32_t* cnt, uint32_t stride,
                                     float* value, float* gathered, float* aux, int routing) {
    HIP_CHECK(hipSetDevice(device_));
    const size_t B = design_.batch;
    if (n_valid < 0 || size_t(n_valid) > B) throw std::invalid_argument("n_valid out of range");
    if (stride == 0) throw std::invalid_argument("gather stride must be positive");
    if (layout_channels(layout) != design_.nb_input_channels)
        throw std::invalid_argument("plane layout has " + std::to_string(layout_channels(layout)) + " channels, net expects " +
                                    std::to_string(design_.nb_input_channels));
    if (!experts_.empty()) {
        submit_boards_gathered_routed(descs_host, n_valid, layout, idx, cnt, stride, value, gathered, aux, routing);
        return;
    }
    if (n_valid > 0 && n_valid <= kBoardSplitMaxBatch && small_path_ok()) {          // few boards on a net made for many: the companion net
        small_net().submit_boards_gathered(descs_host, n_valid, layout, idx, cnt, stride, value, gathered, aux);
        return;
    }
    // No copy commands at all: the descriptors and the gather lists are read by the kernels straight from the caller's pinned
    // (device-visible, coherent) buffers, and the gather kernel writes values, gathered priors and aux straight into them.  A batch
    // moves ~50 KB in and ~170 KB out, so PCIe bandwidth is irrelevant; what a copy costs is the hand-over between the DMA engine
    // and the compute queue -- five copies around three kernel groups were 0.1-0.5 ms of latency per batch (host dependent), more
    // than the forward itself on a loaded host.  One queue, three launches back to back; the host polls the stream.
    Impl& im = *impl_;
    const char lane_mode_c[2] = {dev_.lane_launches, 0};             // CRA_LANE_LAUNCHES "1" / "2" / "3": force the shape of the lane step
    const char* lane_mode = dev_.lane_launches ? lane_mode_c : nullptr;
    if (im.ops.size() == 1 && im.ops[0].kind == OpKind::Forward && !(lane_mode && lane_mode[0] == '3')) {
        // The forward kernel's head writes the gathered priors, value and aux of a board straight into the caller's buffers: a search
        // reads nothing else (set_probabilities_for_moves, node.cpp:961-979), so neither the 20.7 KB probability vector nor the logits of
        // a board leave its CU, and there is no gather launch behind the forward.
        //  * SMALL batches, where the launches themselves are what a lane step costs (a batch of 8 occupies 8 CUs for 0.1 ms), run as
        //    ONE launch: the kernel's stem builds the planes of a board from its descriptor (profiles/r02/t_*: single-tree search at
        //    batch 8 +4-5 % with 1 to 8 collectors).
        //  * LARGE batches keep the plane builder as a launch of its own: inside the 0.31 ms kernel it cost more than the small launch
        //    does beside the other lane's forward (-4 % on the headline search leg).
        const bool one_launch = lane_mode ? lane_mode[0] == '1' : B <= 64;
        const Op& op = im.ops[0];
        StemArgs st = op.st;
        HeadArgs h = op.hd;
        if (one_launch) {
            st.descs = descs_host;
            st.layout = layout;
            st.n_valid = n_valid;
        } else if (n_valid > 0) {
            launch_planes_from_desc(static_cast<const BoardDesc*>(descs_host), n_valid, layout, 1, d_planes_, stream_);
        }
        h.value = value;
        h.probs = nullptr;
        h.logits = nullptr;
        h.aux = (d_aux_ && aux) ? aux : d_aux_;
        h.g_idx = idx;
        h.g_cnt = cnt;
        h.g_out = gathered;
        h.g_stride = int(stride);
        h.g_n_valid = n_valid;
        touch_stream();
        Turn turn(*this);                         // forwards that fill the chip take turns (small batches: a no-op)
        launch_forward(st, op.tw, h, stream_);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (n_valid > 0) launch_planes_from_desc(static_cast<const BoardDesc*>(descs_host), n_valid, layout, 1, d_planes_, stream_);
    // (this net as the companion of a larger one, or any small-batch net with fewer valid boards than its batch: a forward of n_valid boards)
    dyn_n_ = (n_valid > 0 && prec_.x3() && prec_.board_split && design_.batch <= kBoardSplitMaxBatch && size_t(n_valid) < B && !dev_.no_small_path) ? n_valid : 0;
    launch_forward_in_stream();
    dyn_n_ = 0;
    if (dev_.lane_sync) HIP_CHECK(hipStreamSynchronize(stream_));     // development: bisecting the lane step's ordering
    launch_gather_probs(d_probs_, design_.nb_policy, idx, cnt, int(stride), n_valid, gathered, d_value_, value, int(B),
                        (d_aux_ && aux) ? d_aux_ : nullptr, aux, stream_);
}

// ---- routed batches: an expert set (one net per game phase behind one handle) ----
// Every board of a call is evaluated by the net of ITS game phase.  The forward is one workgroup per board and boards never meet inside
// it, so 256 boards split over three experts are still 256 workgroups -- three launches of n_e workgroups each instead of one of 256.
// Per call the HOST derives the phases from the descriptors (desc_game_phase), groups the board indices by expert (stable) and writes the
// list into a pinned buffer of the set: it needs the counts to size the launches, so grouping on the device would only add a
// synchronisation.  Expert e then runs, in ITS stream (the library's per-queue streams: the groups share the chip instead of queueing),
//   planes_from_desc_indexed (slot w <- descriptor board_of[w])  ->  its own forward over n_e boards  ->  gather_probs_indexed
// (slot w's priors / value / aux -> board board_of[w]'s places in the caller's pinned buffers).  A group of at most 64 boards goes where a
// plain net sends it (the companion net's split-board forward), a larger one runs the full-size net's launches on n_e workgroups
// (dyn_n_).  The tower, block, conv and head kernels are the plain net's: a board's numbers depend on its expert's weights and on
// nothing else.  Fork and join are events; the host waits for nothing between the groups, and a routed call is ONE turn (Turn).
namespace {
struct HostDesign { int cin = 0, policy = 0, aux = 0, version = 0; };
HostDesign host_design(const std::string& dir, int batch_size) {
    const std::string file = find_model_file(dir, batch_size);
    NetFile nf;
    if (file.size() > 5 && file.compare(file.size() - 5, 5, ".onnx") == 0) import_onnx(dir + file, nf);
    else nf.load(dir + file);
    HostDesign d;
    d.cin = int(nf.num("nb_input_channels"));
    d.policy = nf.num("select_policy_from_plane", 1) != 0 ? int(nf.num("channels_policy_head")) * kSquares : int(nf.num("n_labels", 0));
    d.aux = (nf.num("use_wdl") != 0 && nf.num("use_plys_to_end") != 0) ? 4 : 0;
    d.version = read_version_from_string(file);
    return d;
}
}  // namespace

std::vector<ExpertDir> discover_experts(const std::string& model_dir, int batch_size, int definition) {
    if (model_dir.empty()) throw std::invalid_argument("The given directory must not be empty.");
    if (definition != PHASE_LICHESS && definition != PHASE_MOVECOUNT)
        throw std::invalid_argument("game phase definition " + std::to_string(definition) + ": 0 lichess, 1 movecount");
    const std::string root = model_dir.back() == '/' ? model_dir : model_dir + "/";
    std::vector<std::string> names;
    if (DIR* d = opendir(root.c_str())) {
        while (dirent* e = readdir(d)) names.emplace_back(e->d_name);
        closedir(d);
    } else {
        throw std::invalid_argument("The given directory at " + root + " cannot be opened");
    }
    std::sort(names.begin(), names.end());
    auto has_ext = [](const std::string& f, const char* ext) { const size_t n = strlen(ext); return f.size() > n && f.compare(f.size() - n, n, ext) == 0; };
    std::vector<ExpertDir> found;
    for (const std::string& n : names) {
        if (n == "." || n == "..") continue;
        struct stat st;
        if (stat((root + n).c_str(), &st) != 0) continue;
        if (!S_ISDIR(st.st_mode)) {
            if (has_ext(n, ".cranet") || has_ext(n, ".onnx"))
                throw std::invalid_argument("The given directory at " + root + " holds the model file " + n + " itself: that is a single net, not a set of game-phase experts -- use mi_net_create");
            continue;
        }
        if (!std::isdigit(static_cast<unsigned char>(n.back()))) continue;           // "phaseNone" and the like
        ExpertDir e;
        e.dir = root + n + "/";
        e.phase = read_game_phase_from_string(e.dir);
        found.push_back(e);
    }
    if (found.empty()) throw std::invalid_argument("The given directory at " + root + " holds no game-phase subdirectory (a name that ends in the phase digit, e.g. phase0)");
    const int n = int(found.size());
    std::vector<const ExpertDir*> by_phase(size_t(n), nullptr);
    for (const ExpertDir& e : found) {
        if (e.phase < n && by_phase[size_t(e.phase)])
            throw std::invalid_argument("The given directory at " + root + " holds game phase " + std::to_string(e.phase) + " twice: " + by_phase[size_t(e.phase)]->dir + " and " + e.dir);
        if (e.phase < n) by_phase[size_t(e.phase)] = &e;
    }
    for (const ExpertDir& e : found)
        if (e.phase >= n) {
            int missing = 0;
            while (missing < n && by_phase[size_t(missing)]) ++missing;
            throw std::invalid_argument("The given directory at " + root + " holds " + std::to_string(n) + " expert(s) but " + e.dir + " is for game phase " + std::to_string(e.phase) +
                                        ": the phases must be 0 .. " + std::to_string(n - 1) + ", phase " + std::to_string(missing) + " is missing");
        }
    if (definition == PHASE_LICHESS && n != 3)
        throw std::invalid_argument("The given directory at " + root + " holds " + std::to_string(n) + " expert(s): the lichess game-phase definition has three phases (board.cpp:544)");
    std::vector<ExpertDir> out;
    for (const ExpertDir* e : by_phase) out.push_back(*e);
    const HostDesign d0 = host_design(out[0].dir, batch_size);
    for (size_t i = 1; i < out.size(); ++i) {
        const HostDesign d = host_design(out[i].dir, batch_size);
        auto differ = [&](const char* what, int a, int b) {
            if (a != b)
                throw std::invalid_argument("The experts of " + root + " disagree in " + what + ": " + out[0].dir + " has " + std::to_string(a) + ", " + out[i].dir + " has " + std::to_string(b));
        };
        differ("input channels", d0.cin, d.cin);
        differ("policy size", d0.policy, d.policy);
        differ("aux outputs", d0.aux, d.aux);
        differ("version", d0.version, d.version);
    }
    return out;
}

struct RiseNet::Group {
    const int* board_of = nullptr;     // the group's boards (indices into the batch), device-visible
    int n = 0;
    int layout = 0;
    const void* descs = nullptr;       // the batch's descriptors (device-visible), or
    const float* planes = nullptr;     // the batch's float planes on the device (predict_routed)
    const uint16_t* idx = nullptr;     // gathered form: the batch's index lists and where the priors go
    const uint32_t* cnt = nullptr;
    uint32_t stride = 0;
    float* gathered = nullptr;
    float* probs = nullptr;            // whole-vector form: the batch's tensors
    float* logits = nullptr;
    float* value = nullptr;            // [batch], [batch][4] or null
    float* aux = nullptr;
};

RiseNet::RiseNet(ExpertSet, const std::string& model_dir, int device_id, int batch_size, const std::string& precision, int game_phase_definition)
    : device_(device_id), impl_(new Impl) {
    if (batch_size <= 0) throw std::invalid_argument("batch size must be positive");
    precision_arg_ = precision;
    prec_ = parse_precision(precision);
    // (every kernel-family suffix too: "-1wg", "-3k", "-8w", "-1b" / "-2b", "-unfused", "-perblock" are A/B variants no routed call was checked in)
    if (prec_.mode != Precision::Mode::Float16x3 || !prec_.fused || !prec_.tower || !prec_.one_launch || prec_.thin_waves || !prec_.board_split || prec_.boards_per_wg != 0)
        throw std::invalid_argument("an expert set runs Precision float16x3 (got '" + precision + "'): the routed forward is checked bit for bit in that mode only");
    const std::vector<ExpertDir> dirs = discover_experts(model_dir, batch_size, game_phase_definition);      // host only: refusals come before the device is touched
    phase_definition_ = game_phase_definition;
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) throw std::invalid_argument("device id out of range");
    HIP_CHECK(hipSetDevice(device_id));
    for (const ExpertDir& d : dirs) experts_.emplace_back(new RiseNet(d.dir, device_id, batch_size, precision));
    design_ = experts_[0]->design_;
    design_.game_phase = 0;
    cu_count_ = experts_[0]->cu_count_;
    model_name_ = experts_[0]->model_name_;
    model_file_path_ = model_dir;
    if (dev_.own_stream || device_id >= 64) HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    else stream_slot_ = take_net_stream(device_id, &stream_);
    const size_t B = size_t(batch_size);
    d_desc_ = impl_->dalloc(B * sizeof(BoardDesc));
    d_planes_ = static_cast<float*>(impl_->dalloc(B * design_.nb_input_channels * kSquares * sizeof(float)));
    d_value_ = static_cast<float*>(impl_->dalloc(B * sizeof(float)));
    d_probs_ = static_cast<float*>(impl_->dalloc(B * design_.nb_policy * sizeof(float)));
    d_logits_ = static_cast<float*>(impl_->dalloc(B * design_.nb_policy * sizeof(float)));
    if (design_.nb_aux) d_aux_ = static_cast<float*>(impl_->dalloc(B * 4 * sizeof(float)));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&route_), (B + experts_.size() + 1) * sizeof(int), hipHostMallocDefault));
    HIP_CHECK(hipEventCreateWithFlags(&fork_ev_, hipEventDisableTiming));
    join_ev_.assign(experts_.size(), nullptr);
    for (hipEvent_t& e : join_ev_) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

void RiseNet::refuse_on_expert_set(const char* what, const char* why) const {
    if (!experts_.empty())
        throw std::invalid_argument(std::string(what) + " on an expert set: " +
                                    (why ? why : "the set has no launches of its own, its experts run the forward -- make the expert's directory a plain net (mi_net_create) for this"));
}

void RiseNet::set_expert_routing(int routing) {
    if (experts_.empty()) throw std::invalid_argument("expert routing: this net is no expert set");
    if (routing != ROUTE_PER_BOARD && routing != ROUTE_MAJORITY) throw std::invalid_argument("expert routing: 0 per board, 1 majority");
    routing_ = routing;
}

void RiseNet::route_phases(const void* descs_host, int n_valid, int* phases_out, int routing) const {
    if (experts_.empty()) throw std::invalid_argument("this net is no expert set");
    if (n_valid < 0 || n_valid > design_.batch) throw std::invalid_argument("n_valid out of range");
    if (routing < 0) routing = routing_;               // (the set's own, mi_net_set_expert_routing; a search lane names its settings' per call)
    if (routing != ROUTE_PER_BOARD && routing != ROUTE_MAJORITY) throw std::invalid_argument("expert routing: 0 per board, 1 majority");
    const BoardDesc* d = static_cast<const BoardDesc*>(descs_host);
    const int E = num_experts();
    int count[10] = {};
    for (int b = 0; b < n_valid; ++b) {
        const int p = std::min(desc_game_phase(d[b], E, phase_definition_), E - 1);
        phases_out[b] = p;
        ++count[p];
    }
    if (routing == ROUTE_MAJORITY && n_valid > 0) {
        // SearchThread::select_nn_index (searchthread.cpp:386-401): std::max_element over the std::map of the phases that occur -- the
        // first of the largest counts, i.e. the lowest phase among ties
        int best = -1;
        for (int p = 0; p < E; ++p)
            if (count[p] > 0 && (best < 0 || count[p] > count[best])) best = p;
        for (int b = 0; b < n_valid; ++b) phases_out[b] = best;
    }
}

// route_ <- the boards 0 .. n - 1 grouped by expert (ascending board index inside a group), then the experts' offsets
void RiseNet::group_boards(const int* phases, int n) {
    const int E = num_experts();
    int* off = route_ + design_.batch;
    for (int e = 0; e <= E; ++e) off[e] = 0;
    for (int b = 0; b < n; ++b) {
        if (phases[b] < 0 || phases[b] >= E) throw std::invalid_argument("board " + std::to_string(b) + " has game phase " + std::to_string(phases[b]) + ", the set has " + std::to_string(E) + " experts");
        ++off[phases[b] + 1];
    }
    for (int e = 0; e < E; ++e) off[e + 1] += off[e];
    int fill[10];
    for (int e = 0; e < E; ++e) fill[e] = off[e];
    for (int b = 0; b < n; ++b) route_[fill[phases[b]]++] = b;
}

void RiseNet::run_group(const Group& g) {
    if (g.n <= kBoardSplitMaxBatch && small_path_ok()) {           // few boards on a net made for many: the companion net, as a plain call
        small_net().run_group(g);
        return;
    }
    if (g.descs) launch_planes_from_desc_indexed(static_cast<const BoardDesc*>(g.descs), g.board_of, g.n, g.layout, 1, d_planes_, stream_);
    else launch_gather_planes_indexed(g.planes, g.board_of, g.n, design_.nb_input_channels * kSquares, d_planes_, stream_);
    // a forward of g.n boards: the companion net's launches take the boards of the call already, the full-size net's the same way
    // (launch_op: every board-batched launch is one workgroup -- or a fixed number of them -- per board)
    dyn_n_ = (g.n < design_.batch && !dev_.no_small_path) ? g.n : 0;
    touch_stream();
    forward_on(stream_);               // (no Turn: the groups of one routed call run side by side, the SET takes the turn)
    dyn_n_ = 0;
    float* aux_dev = (d_aux_ && g.aux) ? d_aux_ : nullptr;
    if (g.gathered)
        launch_gather_probs_indexed(d_probs_, design_.nb_policy, g.idx, g.cnt, int(g.stride), g.board_of, g.n, g.gathered, d_value_, g.value, aux_dev, g.aux, stream_);
    else
        launch_scatter_rows_indexed(d_probs_, g.logits ? d_logits_ : nullptr, design_.nb_policy, g.board_of, g.n, g.probs, g.logits, d_value_, g.value, aux_dev, g.aux, stream_);
    HIP_CHECK(hipGetLastError());
}

void RiseNet::routed_call(int n_valid, const Group& proto) {
    (void)n_valid;
    const int* off = route_ + design_.batch;
    touch_stream();
    Turn turn(*this);                  // one routed call is one turn: whatever fills the chip before it is in front of ALL its groups
    HIP_CHECK(hipEventRecord(fork_ev_, stream_));
    for (int e = 0; e < num_experts(); ++e) {
        const int n_e = off[e + 1] - off[e];
        if (n_e == 0) continue;
        RiseNet& x = *experts_[size_t(e)];
        HIP_CHECK(hipStreamWaitEvent(x.stream_, fork_ev_, 0));
        Group g = proto;
        g.board_of = route_ + off[e];
        g.n = n_e;
        x.run_group(g);
        HIP_CHECK(hipEventRecord(join_ev_[size_t(e)], x.stream_));
        HIP_CHECK(hipStreamWaitEvent(stream_, join_ev_[size_t(e)], 0));
    }
}

void RiseNet::submit_boards_routed(const void* descs_host, int n_valid, int layout, float* value, float* probs, float* aux, int routing) {
    if (n_valid == 0) return;
    std::vector<int> phases(static_cast<size_t>(n_valid));
    route_phases(descs_host, n_valid, phases.data(), routing);
    group_boards(phases.data(), n_valid);
    HIP_CHECK(hipMemcpyAsync(d_desc_, descs_host, size_t(n_valid) * sizeof(BoardDesc), hipMemcpyHostToDevice, stream_));
    Group g;
    g.layout = layout;
    g.descs = d_desc_;
    g.probs = d_probs_;
    g.logits = keep_logits_ ? d_logits_ : nullptr;
    g.value = d_value_;
    g.aux = d_aux_;
    routed_call(n_valid, g);
    const size_t rows = size_t(n_valid);
    HIP_CHECK(hipMemcpyAsync(value, d_value_, rows * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(probs, d_probs_, rows * design_.nb_policy * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (d_aux_ && aux) HIP_CHECK(hipMemcpyAsync(aux, d_aux_, rows * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
}

void RiseNet::submit_boards_gathered_routed(const void* descs_host, int n_valid, int layout, const uint16_t* idx, const uint32_t* cnt, uint32_t stride,
                                            float* value, float* gathered, float* aux, int routing) {
    if (n_valid == 0) return;
    std::vector<int> phases(static_cast<size_t>(n_valid));
    route_phases(descs_host, n_valid, phases.data(), routing);
    group_boards(phases.data(), n_valid);
    // no copy commands, as on a plain net: descriptors, index lists and results stay in the caller's pinned buffers
    Group g;
    g.layout = layout;
    g.descs = descs_host;
    g.idx = idx;
    g.cnt = cnt;
    g.stride = stride;
    g.gathered = gathered;
    g.value = value;
    g.aux = (d_aux_ && aux) ? aux : nullptr;
    routed_call(n_valid, g);
}

void RiseNet::predict_routed(const float* in_planes, const int* phases, float* value, float* probs, float* aux) {
    if (experts_.empty()) throw std::invalid_argument("mi_net_predict_routed: this net is no expert set");
    HIP_CHECK(hipSetDevice(device_));
    const size_t B = design_.batch;
    group_boards(phases, int(B));
    HIP_CHECK(hipMemcpyAsync(d_planes_, in_planes, B * design_.nb_input_channels * kSquares * sizeof(float), hipMemcpyHostToDevice, stream_));
    Group g;
    g.planes = d_planes_;
    g.probs = d_probs_;
    g.logits = keep_logits_ ? d_logits_ : nullptr;
    g.value = d_value_;
    g.aux = d_aux_;
    routed_call(int(B), g);
    HIP_CHECK(hipMemcpyAsync(value, d_value_, B * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(probs, d_probs_, B * design_.nb_policy * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (d_aux_ && aux) HIP_CHECK(hipMemcpyAsync(aux, d_aux_, B * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
    wait();
}

void RiseNet::wait() {
    struct Done {                                                       // the predict is over however this call ends
        RiseNet& n;
        ~Done() {
            if (n.counted_in_flight_) {
                g_predicts_in_flight[n.device_].fetch_sub(1, std::memory_order_relaxed);
                n.counted_in_flight_ = false;
            }
        }
    } done{*this};
    // CRA_WAIT_POLL=1 polls hipStreamQuery instead (development: on the hosts measured so far the runtime's own wait was not the
    // source of the per-batch latency; both give the same pipeline rate)
    static const bool poll = getenv("CRA_WAIT_POLL") != nullptr;
    if (poll) {
        for (;;) {
            const hipError_t e = hipStreamQuery(stream_);
            if (e == hipSuccess) return;
            if (e != hipErrorNotReady) HIP_CHECK(e);
            __builtin_ia32_pause();
        }
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
}

void RiseNet::predict(const float* in_planes, float* value, float* probs, float* aux) {
    submit(in_planes, value, probs, aux);
    wait();
}

void* RiseNet::enable_block_dump(int* n_tiles) {
    refuse_on_expert_set("the block dump");
    HIP_CHECK(hipSetDevice(device_));
    Op* tower = nullptr;
    for (Op& op : impl_->ops)
        if (op.kind == OpKind::Tower || op.kind == OpKind::Forward) {
            if (tower) throw std::runtime_error("block dump: more than one tower launch in this net");
            tower = &op;
        }
    if (!tower) throw std::runtime_error("block dump: this net / precision does not run the one-launch bottleneck tower");
    const int tiles = tower->tw.nblocks + 1;
    if (!tower->tw.block_dump) {
        HIP_CHECK(hipStreamSynchronize(stream_));
        tower->tw.block_dump = impl_->dalloc(size_t(tiles) * design_.batch * kSquares * 256 * sizeof(half_t));
        if (launches_ > 1) {                 // forwards of several launches replay a captured graph: capture again with the pointer set
            if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
            if (graph_) (void)hipGraphDestroy(graph_);
            graph_exec_ = nullptr;
            graph_ = nullptr;
            capture();
        }
    }
    if (n_tiles) *n_tiles = tiles;
    return tower->tw.block_dump;
}

std::string int8_calibration_path(const std::string& model_file_path) { return model_file_path + ".int8calib"; }

std::vector<std::pair<float, float>> read_int8_calibration(const std::string& model_file_path) {
    std::vector<std::pair<float, float>> out;
    std::ifstream f(int8_calibration_path(model_file_path));
    if (!f) return out;
    std::string magic, word;
    int version = 0, boards = 0, blocks = 0;
    f >> magic >> version >> word >> boards >> word >> blocks;
    if (magic != "crazyara-int8-calibration" || version != 1 || blocks <= 0 || blocks > 4096)
        throw std::runtime_error("malformed INT8 calibration file " + int8_calibration_path(model_file_path));
    for (int i = 0; i < blocks; ++i) {
        float a = 0.f, b = 0.f;
        if (!(f >> a >> b) || !(a >= 0.f) || !(b >= 0.f)) throw std::runtime_error("malformed INT8 calibration file " + int8_calibration_path(model_file_path));
        out.emplace_back(a, b);
    }
    return out;
}

std::vector<std::pair<float, float>> RiseNet::calibration_maxima(const float* planes_host, int n_boards) {
    refuse_on_expert_set("calibration", "an expert set runs Precision float16x3 only");
    if (prec_.fused || !prec_.fp16() || prec_.fp8_tower()) throw std::logic_error("calibration_maxima: a net made with Precision float16-unfused");
    if (!planes_host || n_boards <= 0) throw std::invalid_argument("calibration needs at least one board");
    HIP_CHECK(hipSetDevice(device_));
    Impl& im = *impl_;
    const int B = design_.batch;
    const size_t per_board = size_t(design_.nb_input_channels) * kSquares;
    std::vector<std::pair<float, float>> out;
    std::vector<half_t> host;
    auto absmax = [&](const void* dev, size_t count) {
        host.resize(count);
        HIP_CHECK(hipMemcpy(host.data(), dev, count * sizeof(half_t), hipMemcpyDeviceToHost));
        float m = 0.f;
        for (size_t i = 0; i < count; ++i) m = std::max(m, std::fabs(float(host[i])));
        return m;
    };
    std::vector<float> chunk(size_t(B) * per_board);
    for (int b0 = 0; b0 < n_boards; b0 += B) {
        for (int j = 0; j < B; ++j)                          // the last chunk repeats boards: a maximum does not mind
            std::memcpy(chunk.data() + size_t(j) * per_board, planes_host + size_t((b0 + j) % n_boards) * per_board, per_board * sizeof(float));
        HIP_CHECK(hipMemcpy(d_planes_, chunk.data(), chunk.size() * sizeof(float), hipMemcpyHostToDevice));
        size_t blk = 0;
        for (int k = 0; k < int(im.ops.size()); ++k) {
            launch_op<half_t>(k, stream_);
            HIP_CHECK(hipStreamSynchronize(stream_));
            const Op& op = im.ops[k];
            if (op.kind != OpKind::Depthwise) continue;
            if (k == 0 || im.ops[k - 1].kind != OpKind::Conv || im.ops[k - 1].conv.out != op.x)
                throw std::logic_error("calibration_maxima: a depthwise op without its expand conv in front");
            const Op& ex = im.ops[k - 1];                     // the expand conv has run: its input (the gated stream) is untouched
            const float mx = absmax(ex.conv.x, size_t(B) * kSquares * size_t(ex.conv.cin));
            const float mt = absmax(op.y, size_t(B) * kSquares * size_t(op.C));
            if (blk == out.size()) out.emplace_back(0.f, 0.f);
            out[blk].first = std::max(out[blk].first, mx);
            out[blk].second = std::max(out[blk].second, mt);
            ++blk;
        }
    }
    return out;
}

std::string calibrate_int8(const std::string& model_path, int device_id, const float* planes_host, int n_boards) {
    if (planes_host && n_boards <= 0) throw std::invalid_argument("calibration needs at least one board");
    RiseNet net(model_path, device_id, planes_host ? std::min(n_boards, 64) : 64, "float16-unfused");
    std::vector<float> own;
    if (!planes_host) {
        own = default_calibration_planes(net.design().nb_input_channels, net.design().version, &n_boards);
        planes_host = own.data();
    }
    const std::vector<std::pair<float, float>> mx = net.calibration_maxima(planes_host, n_boards);
    if (mx.empty()) throw std::runtime_error("Precision int8 runs on the one-launch bottleneck tower only: this model has no bottleneck blocks");
    const std::string path = int8_calibration_path(net.model_file_path());
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    f << "crazyara-int8-calibration 1\nboards " << n_boards << "\nblocks " << mx.size() << "\n";
    f.precision(9);
    for (const auto& p : mx) f << p.first << " " << p.second << "\n";
    if (!f) throw std::runtime_error("cannot write " + path);
    return path;
}


}  // namespace cra
