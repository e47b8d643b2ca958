// RiseNet: the MI355X-native executor behind the NeuralNetAPI boundary.
// Lifecycle mirrors TensorrtAPI (engine/src/nn/tensorrtapi.cpp:43-63,160-237): construct on a device with a fixed batch
// size -> load_model (read .cranet) -> init_nn_design (shapes) -> load_parameters (fold BN, pack MFMA fragments, upload)
// -> bind_executor (stream, device buffers, hipGraph capture of the whole forward) -> predict().
#pragma once
#include <hip/hip_runtime.h>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "board_net.h"
#include "netfile.h"

namespace cra {

// the host-side weight quantiser of Precision fp8: float -> OCP e4m3fn byte, round to nearest even, clamped at +-448
uint8_t float_to_e4m3(float v);
uint8_t float_to_e5m2(float v);

// What a precision string selects (parse_precision, precision.cpp): the arithmetic and the kernel-family variants.  Every suffix combines
// with every mode when parsed; "-unfused" also drops the tower.  Which combinations a model can run is decided when the net is built
// (fp8 / int8 need the one-launch bottleneck tower, the suffixes that name a kernel family only act where that family runs).
struct Precision {
    enum class Mode { Float32, Float16, Float16x3, Float16p8, Fp8, Int8 };
    Mode mode = Mode::Float16;
    bool fused = true;         // "-unfused": the layer-granular kernels (A/B reference for the fused block kernel); also no tower
    bool tower = true;         // "-perblock": one launch per bottleneck block (A/B reference for the tower kernel)
    bool one_launch = true;    // stem + tower + head in one launch when the net is exactly that chain ("-3k": three launches)
    bool thin_waves = false;   // dense residual tower: 8 waves x 32 couts ("-8w") instead of 4 x 64
    bool board_split = true;   // float16x3 / float16p8 small batches run split-board blocks ("-1wg": one workgroup per board)
    bool wblock = false;       // "-wblock": float16x3 / float16p8 nets of 128 / 192 / 224 channels run their mobile-bottleneck blocks one launch each
                               // (x3_wblock.cpp: block_x3w_kernel) instead of three layer launches; opt-in, refused where no block qualifies
    bool wnet = false;         // "-wnet": "-wblock" (implied) plus every NextViT transformer block of such a net in one launch (x3_wntb.cpp:
                               // ntb_x3w_kernel) instead of nine; opt-in
    bool wsplit = false;       // "-wsplit": "-wnet" (implied) and, in a net made for at most kBoardSplitMaxBatch boards, every block of "-wblock" over
                               // several workgroups per board (x3_wsplit.cpp: block_x3w_split_kernel); opt-in
    bool wtower = false;       // "-wtower": "-wnet" (implied) and every maximal run of two or more consecutive blocks of "-wblock" in one launch
                               // (x3_wtower.cpp: tower_x3w_kernel), a gated block starting a run; opt-in
    int boards_per_wg = 0;     // dense residual tower: 0 = by batch size (2 from 512 boards), 1 / 2 = forced ("-1b" / "-2b")
    bool fp16() const { return mode == Mode::Float16 || mode == Mode::Fp8 || mode == Mode::Int8; }   // f16 activations (else float)
    bool x3() const { return mode == Mode::Float16x3 || mode == Mode::Float16p8; }    // split-operand f16 MFMAs (x3.hip)
    bool p8() const { return mode == Mode::Float16p8; }       // float16x3 whose tower takes the 1x1 GEMMs' cross terms through e5m2 MFMAs
    bool fp8_tower() const { return mode == Mode::Fp8 || mode == Mode::Int8; }       // 8-bit operands in the tower's GEMMs
    bool int8() const { return mode == Mode::Int8; }           // the calibrated INT8 mode (tower.hip Q = 2)
};
Precision parse_precision(const std::string& precision);   // throws std::invalid_argument

class RiseNet : public BoardNet {
public:
    // model_path: a .cranet file, or a directory searched like get_onnx_model_name() (neuralnetapi.cpp:57-73).
    // precision: "float16" (f16 MFMA operands, f32 accumulate; the reference TensorRT default, optionsuci.cpp:143-147)
    //            or "fp8" ("float8"; "int8" is accepted as the reference's name for its reduced-precision mode): float16 with e4m3
    //            operands in the GEMMs of the residual tower (256-channel bottleneck nets only)
    //            or "float16x3" (float activations, every dense contraction as three f16 MFMAs on hi/lo split operands: ~1e-5 on the
    //            logits at several times the float32 rate, x3.hip)
    //            or "float32" (exact f32 MFMA); float16 runs the residual tower kernel (tower.hip: runs of 3x3 blocks in one launch);
    //            suffix "-perblock" selects one fused launch per bottleneck block, "-unfused" the layer-granular kernels
    //            (both kept for A/B measurements and as independent implementations in the parity tests); "-wblock" on float16x3 /
    //            float16p8 runs the mobile-bottleneck blocks of a 128 / 192 / 224-channel net (AlphaVile) one launch each, "-wnet" its
    //            transformer blocks too, "-wsplit" is "-wnet" with those blocks over several workgroups per board in a net made for at
    //            most kBoardSplitMaxBatch boards, "-wtower" is "-wnet" with every run of consecutive such blocks in one launch.   Throws std::invalid_argument / std::runtime_error.
    RiseNet(const std::string& model_path, int device_id, int batch_size, const std::string& precision) : RiseNet(model_path, device_id, batch_size, precision, nullptr) {}
    ~RiseNet() override;

    const std::string& model_file_path() const { return model_file_path_; }
    bool fp16() const { return prec_.fp16(); }
    int cu_count() const { return cu_count_; }

    // NeuralNetAPI::predict contract (neuralnetapi.h:230-237): whole fixed batch, host pointers, blocking;
    // value after tanh, policy after softmax over all nb_policy entries.
    void predict(const float* in_planes, float* value, float* probs, float* aux);
    // asynchronous split of the same call: submit() enqueues H2D + forward + D2H on the net's side stream and returns;
    // wait() blocks until results are in the host buffers.  Host buffers should come from mi_host_alloc (pinned).
    void submit(const float* in_planes, float* value, float* probs, float* aux);
    void wait() override;
    // the descriptor-fed calls (board_net.h); `routing` is ignored
    void submit_boards(const void* descs_host, int n_valid, int layout, float* value, float* probs, float* aux, int routing = -1) override;
    void submit_boards_gathered(const void* descs_host, int n_valid, int layout, const uint16_t* idx, const uint32_t* cnt, uint32_t stride,
                                float* value, float* gathered, float* aux, int routing = -1) override;
    // What one expert of a routed call is handed (expert_set.hip): run_group builds the planes of the group's boards, runs a forward of
    // g.n boards in this net's stream and sends the results to the boards' own slots of the batch.  No wait, no turn: the set takes it.
    struct Group {
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
    void run_group(const Group& g);

    // INT8 calibration (the reference: Int8EntropyCalibrator2 over ChessBatchStream, tensorrtapi.cpp:334-360): on a net made with Precision
    // "float16-unfused" -- every tensor of a block passes through HBM there -- runs the n boards (float planes, NCHW, as predict() takes
    // them) and returns per bottleneck block the largest |value| of the (gated) stream in front of it and of its depthwise output.
    std::vector<std::pair<float, float>> calibration_maxima(const float* planes_host, int n_boards);

    // the one-launch head also writes policy_out (pre-softmax) to d_logits() (parity tests); nets whose heads run as separate launches
    // always have it there (the softmax launch reads it)
    void keep_logits(bool on) override;
    // test hook: the one-launch bottleneck tower also stores the f16 residual stream in front of its first block and behind every
    // block (kernels.h: TowerArgs::block_dump).  Returns the device buffer [n_tiles][B][64][256] f16; throws when the net has no such
    // tower (or more than one run of blocks).
    void* enable_block_dump(int* n_tiles);
    void dev_launch_op(int op, int iters);                        // development: op `op` of the forward `iters` times into the net's stream, no wait
    float* value_head_debug() const { return value_head_dbg_; }   // development: [B][8] stage checksums (CRA_VALUE_HEAD_DEBUG), else null
    // development: the co-residency screen (scripts/coresidency_screen.py, profiles/NOTES.md round 5).  prepare: with a forward of
    // OTHER planes behind it, runs the forward op by op and records, per op, which of the net's mutable device buffers it changes, their
    // contents before and after, and whether the op gives the same bits when launched again on its own output (else its buffers are put
    // back before every launch).  run: op `op` alone `launches` times on the net's stream, every launch compared word for word on the
    // device with the recorded result; returns the number of launches that differed (words: how many 16-byte pieces in all).
    int dev_screen_prepare();
    long dev_screen_run(int op, int launches, long* words);
    std::string dev_screen_info(int op) const;
    void forward_async();                // graph replay on stream(); no copies, no sync

    // per-launch bookkeeping (bench.py roofline: live hipEvent timing of each op on the net stream)
    int launches_per_forward() const { return launches_; }
    const char* op_name(int i) const;
    const char* op_kernel(int i) const;                // the kernel op i launches where one op name covers several (tower_x3: launch_tower_x3's choice; float16x3's policy chain: conv3x3_x3_chain_kernel or, with the value head on its idle waves, conv3x3_x3_heads_kernel), else op_name(i)
    void time_ops(int iters, float* ms);               // ms[i] += elapsed of op i, summed over iters (un-graphed launches)
    float time_forward(int iters);                     // graph replays between two events, returns ms

    // predict()/submit() with ALL of the caller's buffers in pinned host memory (mi_host_alloc / hipHostMalloc / hipHostRegister, as
    // NeuralNetAPIUser allocates them under its TENSORRT branch, neuralnetapiuser.cpp:50-60): no copy commands -- the first kernel reads
    // the planes and the last kernels write value / probabilities / aux straight through PCIe, one queue, nothing handed to the DMA
    // engines and back.  Pageable buffers keep the three hipMemcpyAsync.  CRA_PREDICT_COPY=1 forces the copies (A/B measurements).
    struct IoOverride {
        const float* planes = nullptr;
        float* value = nullptr;
        float* probs = nullptr;
        float* aux = nullptr;
    };
    bool last_submit_was_zero_copy() const { return last_zero_copy_; }

private:
    friend class ExpertSet;                 // keep_logits reaches an expert's companion net (small_), as run_group does
    // One forward: how many boards it runs and where its input / output tensors are.  Made by whoever starts the forward and handed down
    // to every launch, so nothing about a call outlives it.
    struct ForwardCall {
        int boards = 0;                    // 0: the whole batch; n: a forward of n boards (every board-batched launch takes n)
        const IoOverride* io = nullptr;
        int prev_g = 1;                    // launch_op: the workgroups per board of the BlockX3Split / BlockX3WSplit launch before this one
    };
    // the companion net of `parent` (small_) works in the parent's stream
    RiseNet(const std::string& model_path, int device_id, int batch_size, const std::string& precision, const RiseNet* parent);
    struct Impl;
    template <typename T> struct Builder;   // the stages of build() over one state (rise_net_build.hip)
    template <typename T> void build(const NetFile& nf);
    template <typename T> void enqueue(hipStream_t s, ForwardCall call);
    template <typename T> void launch_op(int i, hipStream_t s, ForwardCall& call);
    void launch_forward_in_stream(ForwardCall call);     // the forward as part of a stream's in-order work (submit*, see rise_net.hip)
    // same forward enqueued kernel-by-kernel on a stream (no graph)
    void forward_on(hipStream_t s, ForwardCall call);
    int boards_of_call(int n_valid) const;                // submit_boards*: a forward of n_valid boards (else 0: the whole batch)
    void capture();
    bool buffers_are_pinned(const float* in_planes, float* value, float* probs, float* aux);
    bool last_zero_copy_ = false;
    bool counted_in_flight_ = false;   // this net's predict is counted in the device's predicts-in-flight (submit ... wait)
    int staged_calls_left_ = 0;        // predict on pinned buffers: calls that still take the staged form after another user was met in flight
    // Development switches: read from the environment ONCE, when the net is constructed -- never on the per-batch path,
    // where several lane threads would otherwise scan `environ` per kernel launch beside a host program that may call setenv.
    struct DevSwitches {
        int conv_dev = -1;              // CRA_X3_CONV_DEV: bisecting switches of conv_gemm_x3_kernel
        bool device_graph = false;      // CRA_DEVICE_GRAPH: replay the graph also for a one-launch forward
        bool lane_graph = false;        // CRA_LANE_GRAPH: the lane step replays the graph
        bool lane_no_graph = false;     // CRA_LANE_NO_GRAPH: the lane step never replays the graph
        bool predict_copy = false;      // CRA_PREDICT_COPY: predict() stages through device buffers also for pinned caller buffers
        bool predict_zero_copy = false; // CRA_PREDICT_ZERO_COPY: predict() on pinned buffers never stages, whatever else is in flight
        char lane_launches = 0;         // CRA_LANE_LAUNCHES: '1' / '2' / '3' force the shape of the lane step
        bool lane_sync = false;         // CRA_LANE_SYNC: a stream sync between forward and gather
        bool x3_symmetric = false;      // CRA_X3_TOWER=symmetric: the float16x3 tower with every wave running all three phases
        int x3_split_dev = 0;           // CRA_X3_SPLIT_DEV: timing switches of block_x3_split_kernel (x3.hip; bits 2 and 4 give wrong results)
        bool no_small_path = false;     // CRA_NO_SMALL_PATH: partial batches run the whole batch's forward as before round 6 (A/B)
        int small_conv_split = 2;       // CRA_SMALL_BATCH_CONV_SPLIT: the wide convs of a small-batch net as 1 = two workgroups of 128 couts per board, 2 = four of 64
        // what build() reads
        bool tower_trace = false;       // CRA_TOWER_TRACE: the tower / head kernels record s_memtime stamps (kernels.h: TowerArgs::trace)
        bool x3_value_one_launch;       // CRA_X3_VALUE_HEAD=one / three: the float16x3 value head as value_head_kernel or three launches
        bool value_head_debug = false;  // CRA_VALUE_HEAD_DEBUG: value_head_kernel's stage checksums (value_head_debug())
        int value_head_lds_pad = -1;    // CRA_VALUE_HEAD_LDS_PAD: kernels.h: ValueHeadArgs::lds_pad
        int value_head_variant = 0;     // CRA_VALUE_HEAD_VARIANT: kernels.h: ValueHeadArgs::variant
        bool x3_no_head_chain = false;  // CRA_X3_NO_HEAD_CHAIN: the float16x3 policy head as two launches
        bool x3_no_tail = false;        // CRA_X3_NO_TAIL: the float16x3 two-role tower runs every chunk at 128 channels (tower_x3_roles_kernel)
        bool x3_no_quad = false;        // CRA_X3_NO_QUAD: the float16x3 two-role tower's 3x3 runs stay on tower_x3_tail_kernel (not tower_x3_quad_kernel)
        bool small_batch_heads_apart = false;   // CRA_SMALL_BATCH_HEADS_APART: a small batch's policy conv and value head as two launches
        bool x3_heads_apart = false;    // CRA_X3_HEADS_APART: the float16x3 policy chain and the value head as two launches also above 64 boards (A/B reference of conv3x3_x3_heads_kernel)
        bool value_head_env = false;    // CRA_X3_VALUE_HEAD or CRA_VALUE_HEAD_VARIANT is set, whatever to: the value head is asked for by kernel, it keeps its own launch
        DevSwitches();
    } dev_;
    float* value_head_dbg_ = nullptr;

    std::string model_file_path_;
    Precision prec_;
    std::vector<std::pair<float, float>> int8_calib_;   // per block: max |stream in front of it|, max depthwise output (read_int8_calibration)
    // Small batches (round 6): float16x3 / float16p8 nets made for at most kBoardSplitMaxBatch boards (64: measured faster up to 96, profiles/r06/d_*) run their 3x3 bottleneck blocks one per
    // launch with up to C_op / 128 workgroups per board (x3.hip: block_x3_split_kernel, float16x3 arithmetic in both modes) instead of the
    // one-workgroup-per-board tower, whose latency a small batch pays in full on a handful of CUs.  "-1wg" after the precision keeps the
    // one-workgroup-per-board tower (A/B, and the parity tests of the tower kernels on the small fixtures).
    static constexpr int kBoardSplitMaxBatch = 64;
    // A net made for MORE boards still meets small batches: the root of a `go` (one board), the first batches of a single tree, the tail of
    // a game loop.  submit_boards / submit_boards_gathered with at most kBoardSplitMaxBatch valid boards go to a companion net of that batch
    // size (same model and precision, made on first use) whose launches take the number of boards of THIS call -- a forward of n boards
    // instead of one of the whole batch (0.33 ms instead of 0.70 for one board of RISEv2-19).  float16x3 / float16p8 only.
    std::unique_ptr<RiseNet> small_;  // works in this net's stream (owns_stream_ = false there)
    bool owns_stream_ = true;         // this net took stream_ itself (from the library's set, or created it: stream_slot_ < 0)
    int stream_slot_ = -1;            // which stream of the library's per-device set this net works in (net_streams.h)
    std::string precision_arg_;       // what the constructor was given (the companion is made with the same)
    int cu_count_ = 256;
    int launches_ = 0;
    hipGraph_t graph_ = nullptr;
    hipGraphExec_t graph_exec_ = nullptr;
    void* d_desc_ = nullptr;
    std::unique_ptr<Impl> impl_;
};

// Precision int8's calibration file beside the model (TensorRT keeps its calibration cache the same way): <model file>.int8calib, text --
// "crazyara-int8-calibration 1", "boards <n>", "blocks <m>", then m lines "<max |stream|> <max depthwise output>".
std::string int8_calibration_path(const std::string& model_file_path);
std::vector<std::pair<float, float>> read_int8_calibration(const std::string& model_file_path);      // empty if the file is missing
// runs the calibration pass (a float16 layer-kernel net of its own on `device_id`) and writes the file; returns its path.
// planes_host == nullptr: the default calibration positions -- the plies of the reference's calibration games (calibration.cpp)
std::string calibrate_int8(const std::string& model_path, int device_id, const float* planes_host, int n_boards);
std::vector<float> default_calibration_planes(int channels, int version, int* n_boards);

}  // namespace cra
