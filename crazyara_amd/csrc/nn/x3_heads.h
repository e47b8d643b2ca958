// Precision float16x3, nets made for more than 64 boards: the policy head's two convs with the board's softmax AND the value head in one
// launch (x3_heads.cpp: conv3x3_x3_heads_kernel).  It is conv3x3_x3_chain_kernel (x3.hip) step for step; the two waves that have no cout
// tile in the second conv (at most six tiles: 96 padded couts) run the value head's conv 1x1 and FC1 meanwhile, and all eight waves its
// last stage.  Policy logits and probabilities have the chain's bits, the value has value_head_kernel_8w's.
#pragma once
#include "kernels.h"

namespace cra {

struct HeadsX3Args {
    ConvArgs conv;          // as launch_conv_gemm_x3 takes the chain (pre_wpk set); conv.x is the board both heads read
    ValueHeadArgs vh;       // the plain tanh head: cv = 8, fc = 256, C = 256, no development switches; vh.x == conv.x, vh.batch == conv.batch
};
bool heads_x3_fits(const ConvArgs& c, const ValueHeadArgs& v);      // what the builder asks before it joins the two ops
void launch_heads_x3(const HeadsX3Args& a, hipStream_t s);
void init_x3_heads_kernel_attributes();
constexpr const char* kHeadsX3KernelName = "conv3x3_x3_heads_kernel";

}  // namespace cra
