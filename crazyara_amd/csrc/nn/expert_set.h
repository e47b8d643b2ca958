// ExpertSet: one net per game phase behind one handle, every board of a call evaluated by the net of ITS phase.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "rise_net.h"

namespace cra {

// One expert of a model directory of game-phase experts: the subdirectory and the phase its name ends in
struct ExpertDir {
    int phase = 0;
    std::string dir;          // with a trailing '/'
};
// Discovery of a phase-expert model directory, host only (fill_nn_vectors, uci/crazyara.cpp:566-600: the subdirectories whose name ends in
// a digit, "phaseNone" and the like skipped; the digit is the phase, neuralnetapi.cpp:229-239) with NeuralNetAPIUser's two asserts
// (neuralnetapiuser.cpp:34-47: phase < number of experts, no phase twice) as refusals, and the agreement of the experts' designs (input
// channels, policy size, aux count, version) read from their model files.  Returns the experts ordered by phase; throws
// std::invalid_argument naming the directory.  definition: 0 lichess (exactly three experts), 1 movecount.
std::vector<ExpertDir> discover_experts(const std::string& model_dir, int batch_size, int game_phase_definition);

// The experts of discover_experts(model_dir), each a RiseNet of its own; the phase of a board comes from its descriptor (desc_game_phase,
// chess/planes.h).  Precision float16x3 only.  submit_boards / submit_boards_gathered / wait work as on a plain net; float planes carry
// no phase, so predict_routed takes the phases from the caller.  The set has no launches of its own: its experts run the forward.
class ExpertSet : public BoardNet {
public:
    ExpertSet(const std::string& model_dir, int device_id, int batch_size, const std::string& precision, int game_phase_definition);
    ~ExpertSet() override;

    int num_experts() const { return int(experts_.size()); }
    enum Routing : int { ROUTE_PER_BOARD = 0, ROUTE_MAJORITY = 1 };      // majority: the reference's rule (SearchThread::select_nn_index)
    void set_expert_routing(int routing);
    int expert_routing() const { return routing_; }
    // routing only: the phase (= expert) every valid board of the call would go to under the set's routing
    void route_phases(const void* descs_host, int n_valid, int* phases_out, int routing = -1) const;
    // the whole fixed batch from float planes, board b on expert phases[b]; blocking, host pointers as RiseNet::predict()
    void predict_routed(const float* in_planes, const int* phases, float* value, float* probs, float* aux);

    void submit_boards(const void* descs_host, int n_valid, int layout, float* value, float* probs, float* aux, int routing = -1) override;
    void submit_boards_gathered(const void* descs_host, int n_valid, int layout, const uint16_t* idx, const uint32_t* cnt, uint32_t stride,
                                float* value, float* gathered, float* aux, int routing = -1) override;
    void wait() override;
    void keep_logits(bool on) override;       // its experts and their companion nets keep them, the set collects the rows in d_logits()

private:
    void group_boards(const int* phases, int n_valid);
    void routed_call(const RiseNet::Group& proto);
    std::vector<std::unique_ptr<RiseNet>> experts_;    // by phase
    int phase_definition_ = 0, routing_ = ROUTE_PER_BOARD;
    // (ONE buffer per set, rewritten at the start of every call: a call must have been waited for before the next one is submitted --
    // the discipline the caller's own pinned buffers ask for anyway)
    int* route_ = nullptr;             // pinned: board_of[batch] (grouped by expert, ascending board index inside a group), then offsets[experts + 1]
    hipEvent_t fork_ev_ = nullptr;
    std::vector<hipEvent_t> join_ev_;
    int stream_slot_ = -1;             // net_streams.h
    int cu_count_ = 256;
    void* d_desc_ = nullptr;           // the staging buffers of the whole-vector forms (d_planes() ... d_aux() are the others)
    struct DeviceAllocs {              // freed with the set, also when its constructor throws
        std::vector<void*> p;
        ~DeviceAllocs() { for (void* a : p) (void)hipFree(a); }
    } allocs_;
};

}  // namespace cra
