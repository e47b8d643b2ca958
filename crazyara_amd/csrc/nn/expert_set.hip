#include "expert_set.h"

#include <algorithm>
#include <cctype>
#include <cstring>
#include <dirent.h>
#include <sys/stat.h>

#include "../chess/planes_host.h"
#include "net_streams.h"
#include "onnx_import.h"
#include "rise_net_impl.h"

namespace cra {

// ---- routed batches: an expert set (one net per game phase behind one handle) ----
// Every board of a call is evaluated by the net of ITS game phase.  The forward is one workgroup per board and boards never meet inside
// it, so 256 boards split over three experts are still 256 workgroups -- three launches of n_e workgroups each instead of one of 256.
// Per call the HOST derives the phases from the descriptors (desc_game_phase), groups the board indices by expert (stable) and writes the
// list into a pinned buffer of the set: it needs the counts to size the launches, so grouping on the device would only add a
// synchronisation.  Expert e then runs, in ITS stream (the library's per-queue streams: the groups share the chip instead of queueing),
//   planes_from_desc_indexed (slot w <- descriptor board_of[w])  ->  its own forward over n_e boards  ->  gather_probs_indexed
// (slot w's priors / value / aux -> board board_of[w]'s places in the caller's pinned buffers).  A group of at most 64 boards goes where a
// plain net sends it (the companion net's split-board forward), a larger one runs the full-size net's launches on n_e workgroups
// (RiseNet::run_group).  The tower, block, conv and head kernels are the plain net's: a board's numbers depend on its expert's weights and on
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

ExpertSet::ExpertSet(const std::string& model_dir, int device_id, int batch_size, const std::string& precision, int game_phase_definition)
    : BoardNet(device_id) {
    if (batch_size <= 0) throw std::invalid_argument("batch size must be positive");
    const Precision prec = parse_precision(precision);
    // (every kernel-family suffix too: "-1wg", "-3k", "-8w", "-1b" / "-2b", "-unfused", "-perblock", "-wblock", "-wnet", "-wsplit", "-wtower" are variants no routed call was checked in)
    if (prec.mode != Precision::Mode::Float16x3 || !prec.fused || !prec.tower || !prec.one_launch || prec.thin_waves || !prec.board_split || prec.boards_per_wg != 0 ||
        prec.wblock || prec.wnet)
        throw std::invalid_argument("an expert set runs Precision float16x3 (got '" + precision + "'): the routed forward is checked bit for bit in that mode only");
    const std::vector<ExpertDir> dirs = discover_experts(model_dir, batch_size, game_phase_definition);      // host only: refusals come before the device is touched
    phase_definition_ = game_phase_definition;
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) throw std::invalid_argument("device id out of range");
    HIP_CHECK(hipSetDevice(device_id));
    for (const ExpertDir& d : dirs) experts_.emplace_back(new RiseNet(d.dir, device_id, batch_size, precision));
    design_ = experts_[0]->design();
    design_.game_phase = 0;
    cu_count_ = experts_[0]->cu_count();
    model_name_ = experts_[0]->model_name();
    stream_ = take_net_stream(device_id, &stream_slot_);
    const size_t B = size_t(batch_size);
    auto dalloc = [&](size_t bytes) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes));
        allocs_.p.push_back(p);
        return p;
    };
    d_desc_ = dalloc(B * sizeof(BoardDesc));
    d_planes_ = static_cast<float*>(dalloc(B * design_.nb_input_channels * kSquares * sizeof(float)));
    d_value_ = static_cast<float*>(dalloc(B * sizeof(float)));
    d_probs_ = static_cast<float*>(dalloc(B * design_.nb_policy * sizeof(float)));
    d_logits_ = static_cast<float*>(dalloc(B * design_.nb_policy * sizeof(float)));
    if (design_.nb_aux) d_aux_ = static_cast<float*>(dalloc(B * 4 * sizeof(float)));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&route_), (B + experts_.size() + 1) * sizeof(int), hipHostMallocDefault));
    HIP_CHECK(hipEventCreateWithFlags(&fork_ev_, hipEventDisableTiming));
    join_ev_.assign(experts_.size(), nullptr);
    for (hipEvent_t& e : join_ev_) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

void ExpertSet::set_expert_routing(int routing) {
    if (routing != ROUTE_PER_BOARD && routing != ROUTE_MAJORITY) throw std::invalid_argument("expert routing: 0 per board, 1 majority");
    routing_ = routing;
}

void ExpertSet::route_phases(const void* descs_host, int n_valid, int* phases_out, int routing) const {
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
void ExpertSet::group_boards(const int* phases, int n) {
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

void ExpertSet::routed_call(const RiseNet::Group& proto) {
    const int* off = route_ + design_.batch;
    touch_net_stream(device_, stream_slot_);
    Turn turn(device_, design_.batch, cu_count_, stream_);                 // one routed call is one turn: whatever fills the chip before it is in front of ALL its groups
    HIP_CHECK(hipEventRecord(fork_ev_, stream_));
    for (int e = 0; e < num_experts(); ++e) {
        const int n_e = off[e + 1] - off[e];
        if (n_e == 0) continue;
        RiseNet& x = *experts_[size_t(e)];
        HIP_CHECK(hipStreamWaitEvent(x.stream(), fork_ev_, 0));
        RiseNet::Group g = proto;
        g.board_of = route_ + off[e];
        g.n = n_e;
        x.run_group(g);
        HIP_CHECK(hipEventRecord(join_ev_[size_t(e)], x.stream()));
        HIP_CHECK(hipStreamWaitEvent(stream_, join_ev_[size_t(e)], 0));
    }
}

void ExpertSet::submit_boards(const void* descs_host, int n_valid, int layout, float* value, float* probs, float* aux, int routing) {
    HIP_CHECK(hipSetDevice(device_));
    check_boards_call(n_valid, layout);
    if (n_valid == 0) return;
    std::vector<int> phases(static_cast<size_t>(n_valid));
    route_phases(descs_host, n_valid, phases.data(), routing);
    group_boards(phases.data(), n_valid);
    HIP_CHECK(hipMemcpyAsync(d_desc_, descs_host, size_t(n_valid) * sizeof(BoardDesc), hipMemcpyHostToDevice, stream_));
    RiseNet::Group g;
    g.layout = layout;
    g.descs = d_desc_;
    g.probs = d_probs_;
    g.logits = keep_logits_ ? d_logits_ : nullptr;
    g.value = d_value_;
    g.aux = d_aux_;
    routed_call(g);
    const size_t rows = size_t(n_valid);
    HIP_CHECK(hipMemcpyAsync(value, d_value_, rows * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(probs, d_probs_, rows * design_.nb_policy * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (d_aux_ && aux) HIP_CHECK(hipMemcpyAsync(aux, d_aux_, rows * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
}

void ExpertSet::submit_boards_gathered(const void* descs_host, int n_valid, int layout, const uint16_t* idx, const uint32_t* cnt, uint32_t stride,
                                       float* value, float* gathered, float* aux, int routing) {
    HIP_CHECK(hipSetDevice(device_));
    check_boards_call(n_valid, layout);
    if (stride == 0) throw std::invalid_argument("gather stride must be positive");
    if (n_valid == 0) return;
    std::vector<int> phases(static_cast<size_t>(n_valid));
    route_phases(descs_host, n_valid, phases.data(), routing);
    group_boards(phases.data(), n_valid);
    // no copy commands, as on a plain net: descriptors, index lists and results stay in the caller's pinned buffers
    RiseNet::Group g;
    g.layout = layout;
    g.descs = descs_host;
    g.idx = idx;
    g.cnt = cnt;
    g.stride = stride;
    g.gathered = gathered;
    g.value = value;
    g.aux = (d_aux_ && aux) ? aux : nullptr;
    routed_call(g);
}

void ExpertSet::predict_routed(const float* in_planes, const int* phases, float* value, float* probs, float* aux) {
    HIP_CHECK(hipSetDevice(device_));
    const size_t B = design_.batch;
    group_boards(phases, int(B));
    HIP_CHECK(hipMemcpyAsync(d_planes_, in_planes, B * design_.nb_input_channels * kSquares * sizeof(float), hipMemcpyHostToDevice, stream_));
    RiseNet::Group g;
    g.planes = d_planes_;
    g.probs = d_probs_;
    g.logits = keep_logits_ ? d_logits_ : nullptr;
    g.value = d_value_;
    g.aux = d_aux_;
    routed_call(g);
    HIP_CHECK(hipMemcpyAsync(value, d_value_, B * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(probs, d_probs_, B * design_.nb_policy * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (d_aux_ && aux) HIP_CHECK(hipMemcpyAsync(aux, d_aux_, B * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
    wait();
}

void ExpertSet::wait() { wait_for_stream(stream_); }

void ExpertSet::keep_logits(bool on) {
    keep_logits_ = on;
    for (auto& e : experts_) {                // its experts (and their companions) keep them, the set collects the rows
        e->keep_logits(on);
        if (e->small_) e->small_->keep_logits(on);
    }
}

ExpertSet::~ExpertSet() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);      // every routed call was joined into stream_
    experts_.clear();
    if (route_) (void)hipHostFree(route_);
    if (fork_ev_) (void)hipEventDestroy(fork_ev_);
    for (hipEvent_t e : join_ev_) (void)hipEventDestroy(e);
    release_net_stream(device_, stream_slot_, stream_);
}

}  // namespace cra
