// What nets of one process share per device (internal to csrc/nn): the streams they work in, the turns their forwards take, and the
// count of predicts in flight.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>

namespace cra {

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
// A net's stream: *slot = which stream of the device's set, or -1 for a stream created for this net alone (CRA_OWN_STREAM_PER_NET, read
// here when the net is made: A/B against the time before the library's streams; or a device id beyond the table).
hipStream_t take_net_stream(int device, int* slot);
void touch_net_stream(int device, int slot);       // the net is submitting work: its stream was used NOW (what the choice for the next new net looks at)
void release_net_stream(int device, int slot, hipStream_t s);     // a drained stream of slot -1 is destroyed; the library's own stay

// Forwards of DIFFERENT streams take turns when a forward fills the chip on its own (one workgroup per board, 160 KiB of LDS: one
// per CU).  Two evaluator lanes (or two NeuralNetAPIUsers) keep two batches in flight on two streams; when the streams sit on
// different hardware queues the dispatcher interleaves the workgroups of both forward kernels, both batches then finish together after
// 2 x 0.31 ms, the host collects for both lanes with nothing queued, and the chip idles for every collect: measured 0.42 ms per batch
// instead of 0.32 on the headline search leg (615k against 750k nodes/s), in one mode or the other for a whole process depending
// on which queues the runtime handed out.  Taking turns (submission order) keeps one batch executing and one queued.  Small batches
// are left alone: a batch of 8 occupies 8 CUs and SHOULD overlap with its neighbour.  The copy path of predict() gains too (its D2H copies
// now run beside the other user's forward: two users 559k -> 767k evals/s); zero-copy predict is exempt (see submit()).
struct ForwardTurns;
struct Turn {
    // the forward of a net made for `batch` boards on a device of `cu_count` CUs, about to be enqueued on `stream`
    Turn(int device, int batch, int cu_count, hipStream_t stream);
    ~Turn();
    Turn(const Turn&) = delete;
    Turn& operator=(const Turn&) = delete;

private:
    ForwardTurns* t = nullptr;
    hipStream_t s = nullptr;
    std::unique_lock<std::mutex> lk;       // a member: released also when the constructor throws
};

// predict()s in flight on a device (submit ... wait of any net): what decides between the two forms of a predict on pinned buffers
// (RiseNet::submit); null for a device id beyond the table
std::atomic<int>* predicts_in_flight(int device);

// blocks until everything enqueued on the stream is done
// CRA_WAIT_POLL=1 polls hipStreamQuery instead (development: on the hosts measured so far the runtime's own wait was not the
// source of the per-batch latency; both give the same pipeline rate)
void wait_for_stream(hipStream_t s);

}  // namespace cra
