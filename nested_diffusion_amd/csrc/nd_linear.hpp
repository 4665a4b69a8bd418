// nd_linear.hpp -- the mapping-MLP chain of nd_linear.hip as the conditioner (nd_conditioner.hip) calls it: library-internal, not part
// of the C ABI.
#pragma once
#include "nd_host.hpp"

// Classifier.forward on packed activations (one input pack, hidden layers written in streaming order)
int nd_mlp_chain(const float* x, const void* const* wpk, const float* const* bias, const int* dims, float* const* hid, float* logits,
                 int M, int dtype, void* ws, size_t ws_bytes, void* stream);
// ... and the same with layers 2..4 of several MLPs sharing launches (their first layers run one by one, each behind its prefix block)
bool nd_mlp_tail_batchable(const int* dims, int M, int nm, int dtype);
int nd_mlp_chain_first(const float* x, const void* w1pk, const float* bias1, const int* dims, float* hid0, int M, int dtype, void* ws,
                       size_t ws_bytes, void* stream);
int nd_mlp_chain_tail(int nm, const nd_mlp_weights* w, const int* dims, float* const* hid0, float* const* hid1, float* const* hid2, float* logits,
                      size_t logits_stride, int M, int dtype, void* stream);
