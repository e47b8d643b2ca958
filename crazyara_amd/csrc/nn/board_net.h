// BoardNet: what a search lane (search/pool.cpp: HipEvaluator) and the C API use on a plain net (rise_net.h: RiseNet) and on a set of
// game-phase experts (expert_set.h: ExpertSet) alike -- the shapes, the stream, the device-side tensors, and the descriptor-fed calls.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../chess/planes.h"

namespace cra {

struct RiseDesign {
    int batch = 0;
    int nb_input_channels = 0;     // C of the [B,C,8,8] input
    int nb_policy = 0;             // policyOutputShape[1]
    int nb_aux = 0;                // auxiliaryOutputShape[1] (0 = none)
    int version = 0;               // make_version(maj,min,0) parsed from the file name (neuralnetapi.cpp:194-227)
    int game_phase = 0;
    double flops_per_position = 0; // 2*MACs, recomputed from the layer list
};

class BoardNet {
public:
    virtual ~BoardNet() = default;
    BoardNet(const BoardNet&) = delete;
    BoardNet& operator=(const BoardNet&) = delete;

    const RiseDesign& design() const { return design_; }
    const std::string& model_name() const { return model_name_; }
    int device() const { return device_; }
    hipStream_t stream() const { return stream_; }

    // descriptor-fed evaluation: 192-byte BoardDesc per position, planes expanded on the GPU (csrc/chess/planes_kernel.hip); enqueued on
    // stream() and returned from, wait() blocks until the results are in the host buffers
    // routing: an expert set's routing for THIS call, -1 = the set's own (ExpertSet::set_expert_routing); plain nets ignore it
    virtual void submit_boards(const void* descs_host, int n_valid, int layout, float* value, float* probs, float* aux, int routing = -1) = 0;
    // the same, but only the probabilities the search will read come back: idx[s * stride .. + cnt[s]) are the policy indices of slot s's
    // legal moves, gathered[] (same layout) receives probs[s][idx].  Every host buffer (descs, idx, cnt, value, gathered, aux) must come
    // from mi_host_alloc / hipHostMalloc: the kernels read and write them in place, there is no copy.
    virtual void submit_boards_gathered(const void* descs_host, int n_valid, int layout, const uint16_t* idx, const uint32_t* cnt, uint32_t stride,
                                        float* value, float* gathered, float* aux, int routing = -1) = 0;
    virtual void wait() = 0;

    // Device-resident path: a forward reads d_planes() and writes d_value()/d_probs()/d_aux()/d_logits().
    float* d_planes() const { return d_planes_; }     // [B][C][64] float (NCHW, as predict() takes it)
    float* d_value() const { return d_value_; }       // [B]
    float* d_probs() const { return d_probs_; }       // [B][nb_policy]
    float* d_logits() const { return d_logits_; }     // [B][nb_policy] pre-softmax policy_out: valid after a forward made with keep_logits(true)
    float* d_aux() const { return d_aux_; }           // [B][nb_aux] or nullptr
    virtual void keep_logits(bool on) = 0;

protected:
    explicit BoardNet(int device_id) : device_(device_id) {}
    void check_boards_call(int n_valid, int layout) const {     // the two submits' argument checks
        if (n_valid < 0 || n_valid > design_.batch) throw std::invalid_argument("n_valid out of range");
        if (layout_channels(layout) != design_.nb_input_channels)
            throw std::invalid_argument("plane layout has " + std::to_string(layout_channels(layout)) + " channels, net expects " +
                                        std::to_string(design_.nb_input_channels));
    }
    RiseDesign design_;
    std::string model_name_;
    int device_ = 0;
    hipStream_t stream_ = nullptr;
    float *d_planes_ = nullptr, *d_value_ = nullptr, *d_probs_ = nullptr, *d_logits_ = nullptr, *d_aux_ = nullptr;
    bool keep_logits_ = false;
};

}  // namespace cra
