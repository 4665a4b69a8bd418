// nd_optim.hpp -- the optimizer update of the training kernels (nd_mlp_train.hip, nd_vit_train.hip, nd_diffusion_train.hip) and the EMA
// shadow's update that can follow it: one element, in registers.
// Every operation is one rounded fp32 op in the listed order (division and square root correctly rounded, denormals kept): a float32
// restatement on the host reproduces it bit for bit (tests/test_gpu_mlp_edges.py, tests/test_gpu_vit_train.py).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nested_diffusion.h"

// the five operations torch 1.10 torch/optim/_functional.py adam and adamw share (no amsgrad); Step: nd_adam_step or nd_adamw_step
template <class Step>
__device__ __forceinline__ void nd_adam_ops(float& w, float& m, float& v, float g, const Step& a) {
#pragma clang fp contract(off)
    m = (m * a.beta1) + (g * a.one_minus_beta1);
    v = (v * a.beta2) + ((g * g) * a.one_minus_beta2);
    const float denom = (sqrtf(v) / a.sqrt_bc2) + a.eps;
    w = w - a.step_size * (m / denom);
}

// adam (no weight decay)
__device__ __forceinline__ void nd_optim_update(float& w, float& m, float& v, float g, const nd_adam_step& a) { nd_adam_ops(w, m, v, g, a); }

// adamw: the decoupled decay first
__device__ __forceinline__ void nd_optim_update(float& w, float& m, float& v, float g, const nd_adamw_step& a) {
#pragma clang fp contract(off)
    w = w * a.decay;
    nd_adam_ops(w, m, v, g, a);
}

// the exponential moving average of a parameter, on the weight the optimizer just wrote (diffusion/ema.py EMA.update: (1 - mu) * param +
// mu * shadow, torch's two scalar products and their sum): three rounded operations, never an fma
__device__ __forceinline__ void nd_ema_update(float& s, float w, const nd_ema_step& e) {
#pragma clang fp contract(off)
    const float pw = e.one_minus_mu * w;
    const float ps = e.mu * s;
    s = pw + ps;
}
