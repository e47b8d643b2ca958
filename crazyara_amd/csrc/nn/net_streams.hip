#include "net_streams.h"

#include <cstdlib>

#include "rise_net_impl.h"

namespace cra {

namespace {
struct NetStreams {
    std::mutex mu;
    int n = 0;
    hipStream_t s[16] = {};
    std::atomic<uint64_t> last[16] = {};
};
NetStreams g_net_streams[64];                  // per device
std::atomic<uint64_t> g_stream_tick{1};
std::atomic<int> g_predicts_in_flight[64];
}  // namespace

hipStream_t take_net_stream(int device, int* slot) {
    hipStream_t out = nullptr;
    if (getenv("CRA_OWN_STREAM_PER_NET") != nullptr || device >= 64) {
        HIP_CHECK(hipStreamCreateWithFlags(&out, hipStreamNonBlocking));
        *slot = -1;
        return out;
    }
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
    *slot = best;
    return ns.s[best];
}

void touch_net_stream(int device, int slot) {
    if (slot >= 0) g_net_streams[device].last[slot].store(g_stream_tick.fetch_add(1, std::memory_order_relaxed), std::memory_order_relaxed);
}

struct ForwardTurns {
    std::mutex mu;
    hipEvent_t ev[64];
    bool made = false, any = false;
    bool multi = false;                   // a second stream has shown up: from then on every forward records its event
    int last = 0;
    hipStream_t last_stream = nullptr;
};
namespace {
ForwardTurns g_turns[64];     // per device
}  // namespace

void release_net_stream(int device, int slot, hipStream_t s) {
    if (!s || slot >= 0) return;
    if (device >= 0 && device < 64) {        // the stream is about to be destroyed (and has been drained): no turn waits for it
        std::lock_guard<std::mutex> lk(g_turns[device].mu);
        if (g_turns[device].last_stream == s) {
            g_turns[device].last_stream = nullptr;
            g_turns[device].any = false;
        }
    }
    (void)hipStreamDestroy(s);
}

Turn::Turn(int device, int batch, int cu_count, hipStream_t stream) {
    static const bool off = getenv("CRA_NO_FORWARD_TURNS") != nullptr;      // development: A/B
    static const bool always = getenv("CRA_FORCE_FORWARD_TURNS") != nullptr;
    if (off || device < 0 || device >= 64 || (!always && batch * 4 < cu_count * 3)) return;
    ForwardTurns* ft = &g_turns[device];
    lk = std::unique_lock<std::mutex>(ft->mu);
    if (!ft->made) {
        HIP_CHECK(hipSetDevice(device));
        for (hipEvent_t& e : ft->ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ft->made = true;
    }
    if (!ft->multi) {
        // one stream on this device so far (a device-resident loop over one net: the headline measurement): nothing to order, and
        // an event record per forward is not free (measured 3 us per 0.33 ms step)
        if (ft->last_stream == nullptr || ft->last_stream == stream) {
            ft->last_stream = stream;
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
    if (ft->any && ft->last_stream != stream) HIP_CHECK(hipStreamWaitEvent(stream, ft->ev[ft->last], 0));
    t = ft;
    s = stream;
}

Turn::~Turn() {
    if (!t) return;
    const int next = (t->last + 1) & 63;
    if (hipEventRecord(t->ev[next], s) == hipSuccess) {
        t->last = next;
        t->last_stream = s;
        t->any = true;
    }
}

std::atomic<int>* predicts_in_flight(int device) { return device >= 0 && device < 64 ? &g_predicts_in_flight[device] : nullptr; }

void wait_for_stream(hipStream_t s) {
    static const bool poll = getenv("CRA_WAIT_POLL") != nullptr;
    if (poll) {
        for (;;) {
            const hipError_t e = hipStreamQuery(s);
            if (e == hipSuccess) return;
            if (e != hipErrorNotReady) HIP_CHECK(e);
            __builtin_ia32_pause();
        }
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace cra
