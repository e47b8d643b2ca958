// Internal to csrc/nn: what the files that make up RiseNet (rise_net.hip, rise_net_build.hip) and the expert set share -- the error
// check, the ops of a forward and the net's device-side state.
#pragma once
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "kernels.h"
#include "rise_net.h"
#include "x3_heads.h"

namespace cra {

#define HIP_CHECK(expr)                                                                                      \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " #expr);      \
    } while (0)

enum class OpKind { PlanesToAct, Conv, Depthwise, SE, ValueHead, Softmax, Block, ValueFinal, SEGate, Tower, Head, Stem, ResTower, Forward, TowerX3, BlockX3Split, X3SplitFinish, HeadsSmall, Attention, BlockX3W, NtbX3W, BlockX3WSplit, X3WSplitFinish, TowerX3W };

struct Op {
    OpKind kind;
    ConvArgs conv{};
    bool from_planes = false;     // float16x3 stem conv: reads the NCHW input planes (their address is a launch-time value too)
    bool fused_softmax = false;   // float16x3 policy-map conv: the softmax runs in its launch (the probabilities' address is a launch-time value)
    bool heads_x3 = false;        // float16x3 policy chain that also runs the value head `vh` (x3_heads.cpp: conv3x3_x3_heads_kernel; Builder::merge_heads_x3)
    // depthwise / se
    const void* x = nullptr;
    void* y = nullptr;
    const float *w0 = nullptr, *w1 = nullptr, *b0 = nullptr;
    int C = 0, ks = 0, se_kind = 0;
    ValueHeadArgs vh{};
    BlockArgs blk{};              // Block; BlockX3W (x3_wblock.cpp)
    NtbArgs ntb{};                // NtbX3W (x3_wntb.cpp)
    ValueFinalArgs vf{};
    TowerArgs tw{};
    HeadArgs hd{};
    ResTowerArgs rt{};
    StemArgs st{};
    X3TowerArgs tx{};
    X3SplitArgs xs{};             // BlockX3Split; X3SplitFinish: x_parts, gin, batch and (xs_y) the float stream
    float* xs_y = nullptr;
    X3WTowerArgs wt{};            // TowerX3W (x3_wtower.cpp); wt.blocks is an upload of the net's (Impl::upload), freed with it
    X3WSplitArgs ws{};            // BlockX3WSplit (x3_wsplit.cpp); X3WSplitFinish: x_parts, gin, blk.C and the float stream blk.y, blk.pool_out
};

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

}  // namespace cra
