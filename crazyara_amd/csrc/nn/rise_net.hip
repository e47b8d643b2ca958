#include "rise_net.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <algorithm>

#include "net_streams.h"
#include "onnx_import.h"
#include "rise_net_impl.h"
#include "../chess/planes_host.h"

namespace cra {

RiseNet::RiseNet(const std::string& model_path, int device_id, int batch_size, const std::string& precision, const RiseNet* parent)
    : BoardNet(device_id), impl_(new Impl) {
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
    if (parent) {                                // the companion net of a larger one works in ITS stream (never at the same time: a call goes to one of them)
        stream_ = parent->stream_;
        stream_slot_ = parent->stream_slot_;
        owns_stream_ = false;
    } else {
        stream_ = take_net_stream(device_id, &stream_slot_);
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
    if (!dev_.no_small_path && prec_.x3() && prec_.tower && prec_.fused && prec_.board_split && design_.batch > kBoardSplitMaxBatch)
        small_.reset(new RiseNet(model_file_path_, device_id, kBoardSplitMaxBatch, precision_arg_, this));
}

RiseNet::~RiseNet() {
    if (counted_in_flight_) predicts_in_flight(device_)->fetch_sub(1, std::memory_order_relaxed);
    (void)hipSetDevice(device_);
    small_.reset();                              // (it works in this net's stream)
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    impl_.reset();
    if (owns_stream_) release_net_stream(device_, stream_slot_, stream_);
}

template <typename T> void RiseNet::launch_op(int i, hipStream_t s, ForwardCall& call) {
    Impl& im = *impl_;
    const int n = call.boards;                                 // > 0: a forward of fewer boards than the net was made for
    const IoOverride* io = call.io;
    const int B = n > 0 ? n : design_.batch;
    const Op& op = im.ops[i];
    auto boards = [&](ConvArgs c) {                            // a board-batched conv of such a forward
        if (n > 0 && c.batch == design_.batch && !c.out_rows_f32) c.batch = n;
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
            if (op.heads_x3) {                               // the policy chain with the value head on its idle waves (x3_heads.cpp)
                HeadsX3Args h;
                h.conv = boards(op.conv);
                h.conv.softmax_out = probs;
                if (!keep_logits_) h.conv.out = nullptr;
                h.vh = op.vh;
                h.vh.value = value;
                h.vh.aux = aux;
                h.vh.batch = h.conv.batch;
                launch_heads_x3(h, s);
            } else if (prec_.x3() && dev_.conv_dev >= 0) {                                // development: bisecting switches of conv_gemm_x3_kernel
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
            if (n > 0) v.batch = n;
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
        case OpKind::BlockX3W: {
            BlockArgs a = op.blk;
            a.batch = B;
            launch_block_x3w(a, s);
            break;
        }
        case OpKind::TowerX3W: {
            X3WTowerArgs a = op.wt;
            a.batch = B;
            launch_tower_x3w(a, s);
            break;
        }
        case OpKind::BlockX3WSplit: {                              // the shares per board follow the boards of THIS forward; a launch reads as
            X3WSplitArgs a = op.ws;                                // many images per board as the launch before it wrote
            if (n > 0) {
                a.blk.batch = n;
                a.G = x3w_split_shares(a.blk.cop_pad, n, cu_count_);
                a.gin = a.stream_in ? 1 : call.prev_g;
                call.prev_g = a.G;
            }
            launch_block_x3w_split(a, s);
            break;
        }
        case OpKind::X3WSplitFinish:
            launch_x3w_split_finish(op.ws.x_parts, n > 0 ? call.prev_g : op.ws.gin, static_cast<float*>(op.ws.blk.y), op.ws.blk.pool_out, B, op.ws.blk.C, s);
            break;
        case OpKind::NtbX3W: {
            NtbArgs a = op.ntb;
            a.batch = B;
            launch_ntb_x3w(a, s);
            break;
        }
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
            if (n > 0) {
                X3TowerArgs t = op.tx;
                t.batch = n;
                launch_tower_x3(t, s);
            } else launch_tower_x3(op.tx, s);
            break;
        case OpKind::BlockX3Split:
            if (n > 0) {                                         // the workgroups per board follow the boards of THIS forward; a launch reads
                X3SplitArgs a = op.xs;                           // as many images per board as the launch before it wrote
                a.batch = n;
                a.G = std::max(1, std::min(std::min(10, cu_count_ / n), a.blk.cop_pad / block_x3_chunk_channels()));
                a.gin = (i == 0 || im.ops[i - 1].kind != OpKind::BlockX3Split) ? 1 : call.prev_g;      // (a run's first block reads the float stream)
                call.prev_g = a.G;
                launch_block_x3_split(a, s);
            } else launch_block_x3_split(op.xs, s);
            break;
        case OpKind::X3SplitFinish: launch_x3_split_finish(op.xs.x_parts, n > 0 ? call.prev_g : op.xs.gin, op.xs_y, B, s); break;
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
            if (op.C == 256) launch_se_gate(static_cast<const float*>(op.x), static_cast<float*>(op.y), op.se_kind, op.w0, op.w1, op.b0, B, op.C, s);
            else launch_se_gate_w(static_cast<const float*>(op.x), static_cast<float*>(op.y), op.se_kind, op.w0, op.w1, op.b0, B, op.C, s);
            break;
    }
}

template <typename T> void RiseNet::enqueue(hipStream_t s, ForwardCall call) {
    // (Round 6 tried the value head of a small batch on a side stream beside the policy head -- two branches of the captured graph: the
    // forward got SLOWER, 0.354 against 0.335 ms at batch 1, the cross-queue joins cost more than the 24 us they hide: profiles/r06/e_*.)
    call.prev_g = 1;
    for (int i = 0; i < int(impl_->ops.size()); ++i) launch_op<T>(i, s, call);
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
        case OpKind::BlockX3W: return "block_x3w";
        case OpKind::NtbX3W: return "ntb_x3w";
        case OpKind::TowerX3W: return "tower_x3w";
        case OpKind::BlockX3WSplit: return "block_x3w_split";
        case OpKind::X3WSplitFinish: return "x3w_split_finish";
    }
    return "?";
}

const char* RiseNet::op_kernel(int i) const {
    const Op& op = impl_->ops.at(i);
    if (op.kind == OpKind::Conv && op.heads_x3) return kHeadsX3KernelName;
    if (op.kind == OpKind::Conv && prec_.x3() && !op.conv.p8 && op.conv.pre_wpk) return "conv3x3_x3_chain_kernel";      // (launch_conv_gemm_x3's first branch)
    return op.kind == OpKind::TowerX3 ? tower_x3_kernel_name(op.tx) : op_name(i);
}

void RiseNet::time_ops(int iters, float* ms) {
    HIP_CHECK(hipSetDevice(device_));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    const int n = int(impl_->ops.size());
    for (int it = 0; it < iters; ++it)
        for (int i = 0; i < n; ++i) {
            HIP_CHECK(hipEventRecord(e0, stream_));
            ForwardCall call;
            if (prec_.fp16()) launch_op<half_t>(i, stream_, call); else launch_op<float>(i, stream_, call);
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
    const Impl& im = *impl_;
    if (op < 0 || op >= int(im.screen.size())) return "";
    size_t bytes = 0;
    for (const ScreenOp::Buf& b : im.screen[op].writes) bytes += b.bytes;
    return std::string(op_name(op)) + " writes " + std::to_string(im.screen[op].writes.size()) + " buffers / " + std::to_string(bytes) + " bytes" +
           (im.screen[op].idempotent ? "" : ", not idempotent (buffers restored before every launch)");
}

void RiseNet::dev_launch_op(int op, int iters) {
    HIP_CHECK(hipSetDevice(device_));
    if (op < 0 || op >= int(impl_->ops.size())) throw std::invalid_argument("op index out of range");
    ForwardCall call;
    for (int it = 0; it < iters; ++it) {
        if (prec_.fp16()) launch_op<half_t>(op, stream_, call); else launch_op<float>(op, stream_, call);
    }
    HIP_CHECK(hipGetLastError());
}

float RiseNet::time_forward(int iters) {
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
        forward_on(cs, ForwardCall{});
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

void RiseNet::forward_on(hipStream_t s, ForwardCall call) {
    if (prec_.fp16()) enqueue<half_t>(s, call); else enqueue<float>(s, call);
}

// Device-resident replay.  A forward that is ONE kernel gains nothing from a graph (there is no launch sequence to save) and loses the
// graph launch's own cost between consecutive replays: it goes into the stream as a plain launch.  Everything else replays the graph.
// CRA_DEVICE_GRAPH=1 forces the graph (A/B timing).
void RiseNet::forward_async() {
    touch_net_stream(device_, stream_slot_);
    Turn turn(device_, design_.batch, cu_count_, stream_);
    if (launches_ == 1 && !dev_.device_graph) {
        forward_on(stream_, ForwardCall{});
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
void RiseNet::launch_forward_in_stream(ForwardCall call) {
    touch_net_stream(device_, stream_slot_);
    Turn turn(device_, design_.batch, cu_count_, stream_);
    if (call.boards > 0 || (launches_ <= 5 && !dev_.lane_graph) || dev_.lane_no_graph) forward_on(stream_, call);      // (a forward of fewer boards: its own arguments)
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
    HIP_CHECK(hipSetDevice(device_));   // every predict selects its device, tensorrtapi.cpp:198
    const size_t B = design_.batch;
    // Zero-copy or staged?  With pinned buffers the kernels can read the planes and write value / probabilities across PCIe themselves: no
    // copy commands, the best form for ONE user (338k against 331k evals/s at batch 256, profiles/r05/p_*).  With a second user's forward
    // on the device the staged form wins by 6 - 12 % in every measurement (422k against 377k: the copies of one user run on the DMA
    // engines beside the other user's forward, while a zero-copy forward holds its CUs for the whole PCIe write): so the form is chosen
    // from what is in flight when the call arrives -- the reference's default is Threads = 2 (optionsuci.cpp), i.e. two users.
    // CRA_PREDICT_COPY / CRA_PREDICT_ZERO_COPY (when the net was made) force one form.
    std::atomic<int>* in_flight = predicts_in_flight(device_);
    const bool others_in_flight = in_flight && in_flight->load(std::memory_order_relaxed) > (counted_in_flight_ ? 1 : 0);
    if (!counted_in_flight_ && in_flight) {
        in_flight->fetch_add(1, std::memory_order_relaxed);
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
        ForwardCall call;
        call.io = &io;
        forward_on(stream_, call);
        return;
    }
    HIP_CHECK(hipMemcpyAsync(d_planes_, in_planes, B * design_.nb_input_channels * kSquares * sizeof(float), hipMemcpyHostToDevice, stream_));
    launch_forward_in_stream(ForwardCall{});
    HIP_CHECK(hipMemcpyAsync(value, d_value_, B * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(probs, d_probs_, B * design_.nb_policy * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (d_aux_ && aux) HIP_CHECK(hipMemcpyAsync(aux, d_aux_, B * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
}

// a forward of n_valid boards instead of the whole batch?  A small-batch float16x3 / float16p8 net (the companion of a larger one, or any
// net made for at most kBoardSplitMaxBatch boards) with fewer valid boards than its batch: its launches take the boards of the call
int RiseNet::boards_of_call(int n_valid) const {
    const bool partial = n_valid > 0 && prec_.x3() && prec_.board_split && design_.batch <= kBoardSplitMaxBatch && n_valid < design_.batch && !dev_.no_small_path;
    return partial ? n_valid : 0;
}

void RiseNet::submit_boards(const void* descs_host, int n_valid, int layout, float* value, float* probs, float* aux, int) {
    HIP_CHECK(hipSetDevice(device_));
    check_boards_call(n_valid, layout);
    if (n_valid > 0 && n_valid <= kBoardSplitMaxBatch && small_) {         // few boards on a net made for many: the companion net
        small_->submit_boards(descs_host, n_valid, layout, value, probs, aux);      // (into this net's stream: wait() as ever)
        return;
    }
    ForwardCall call;
    call.boards = boards_of_call(n_valid);
    const size_t rows = call.boards ? size_t(call.boards) : size_t(design_.batch);     // (of a partial forward only its boards' results go back)
    if (n_valid > 0) {
        HIP_CHECK(hipMemcpyAsync(d_desc_, descs_host, size_t(n_valid) * sizeof(BoardDesc), hipMemcpyHostToDevice, stream_));
        launch_planes_from_desc(static_cast<const BoardDesc*>(d_desc_), n_valid, layout, 1, d_planes_, stream_);
    }
    launch_forward_in_stream(call);
    HIP_CHECK(hipMemcpyAsync(value, d_value_, rows * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(probs, d_probs_, rows * design_.nb_policy * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (d_aux_ && aux) HIP_CHECK(hipMemcpyAsync(aux, d_aux_, rows * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
}

void RiseNet::submit_boards_gathered(const void* descs_host, int n_valid, int layout, const uint16_t* idx, const uint32_t* cnt, uint32_t stride,
                                     float* value, float* gathered, float* aux, int) {
    HIP_CHECK(hipSetDevice(device_));
    check_boards_call(n_valid, layout);
    if (stride == 0) throw std::invalid_argument("gather stride must be positive");
    const size_t B = design_.batch;
    if (n_valid > 0 && n_valid <= kBoardSplitMaxBatch && small_) {          // few boards on a net made for many: the companion net
        small_->submit_boards_gathered(descs_host, n_valid, layout, idx, cnt, stride, value, gathered, aux);
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
        touch_net_stream(device_, stream_slot_);
        Turn turn(device_, design_.batch, cu_count_, stream_);      // forwards that fill the chip take turns (small batches: a no-op)
        launch_forward(st, op.tw, h, stream_);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (n_valid > 0) launch_planes_from_desc(static_cast<const BoardDesc*>(descs_host), n_valid, layout, 1, d_planes_, stream_);
    ForwardCall call;
    call.boards = boards_of_call(n_valid);
    launch_forward_in_stream(call);
    if (dev_.lane_sync) HIP_CHECK(hipStreamSynchronize(stream_));     // development: bisecting the lane step's ordering
    launch_gather_probs(d_probs_, design_.nb_policy, idx, cnt, int(stride), n_valid, gathered, d_value_, value, int(B),
                        (d_aux_ && aux) ? d_aux_ : nullptr, aux, stream_);
}

void RiseNet::run_group(const Group& g) {
    if (g.n <= kBoardSplitMaxBatch && small_) {                    // few boards on a net made for many: the companion net, as a plain call
        small_->run_group(g);
        return;
    }
    if (g.descs) launch_planes_from_desc_indexed(static_cast<const BoardDesc*>(g.descs), g.board_of, g.n, g.layout, 1, d_planes_, stream_);
    else launch_gather_planes_indexed(g.planes, g.board_of, g.n, design_.nb_input_channels * kSquares, d_planes_, stream_);
    // a forward of g.n boards: the companion net's launches take the boards of the call already, the full-size net's the same way
    // (launch_op: every board-batched launch is one workgroup -- or a fixed number of them -- per board)
    ForwardCall call;
    call.boards = (g.n < design_.batch && !dev_.no_small_path) ? g.n : 0;      // (not boards_of_call: a full-size expert runs g.n workgroups of its big tower)
    touch_net_stream(device_, stream_slot_);
    forward_on(stream_, call);         // (no Turn: the groups of one routed call run side by side, the SET takes the turn)
    float* aux_dev = (d_aux_ && g.aux) ? d_aux_ : nullptr;
    if (g.gathered)
        launch_gather_probs_indexed(d_probs_, design_.nb_policy, g.idx, g.cnt, int(g.stride), g.board_of, g.n, g.gathered, d_value_, g.value, aux_dev, g.aux, stream_);
    else
        launch_scatter_rows_indexed(d_probs_, g.logits ? d_logits_ : nullptr, design_.nb_policy, g.board_of, g.n, g.probs, g.logits, d_value_, g.value, aux_dev, g.aux, stream_);
    HIP_CHECK(hipGetLastError());
}

void RiseNet::wait() {
    struct Done {                                                       // the predict is over however this call ends
        RiseNet& n;
        ~Done() {
            if (n.counted_in_flight_) {
                predicts_in_flight(n.device_)->fetch_sub(1, std::memory_order_relaxed);
                n.counted_in_flight_ = false;
            }
        }
    } done{*this};
    wait_for_stream(stream_);
}

void RiseNet::predict(const float* in_planes, float* value, float* probs, float* aux) {
    submit(in_planes, value, probs, aux);
    wait();
}

void* RiseNet::enable_block_dump(int* n_tiles) {
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

std::vector<std::pair<float, float>> RiseNet::calibration_maxima(const float* planes_host, int n_boards) {
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
        ForwardCall call;
        for (int k = 0; k < int(im.ops.size()); ++k) {
            launch_op<half_t>(k, stream_, call);
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
