// nd_vit.hpp -- what the ViT units share (nd_gemm_nt.hip, nd_gemm_f32.hip, nd_layernorm.hip, nd_attention.hip, nd_attention_b9.hip,
// nd_attention_h.hip, nd_vit_grad.hip): the launchers one unit defines and another calls, the tile constants a launch plan and its kernel must agree on,
// and the two template dispatches.  The defining units include it too, so each signature exists once.
#pragma once
#include <hip/hip_runtime.h>

// ---- large-M GEMM, both operands K-contiguous (plan and fp16 kernel: nd_gemm_nt.hip; fp32 kernel: nd_gemm_f32.hip) ----
#define GB_K 16    // fp32 form: K per stage
#define GB_LD 24   // 16 + 8 pad: ds_read_b128 of (row = l&15, k-quad = l>>4) is bank-conflict-free
#define GH_K 32    // fp16 form: K per stage = one v_mfma_f32_16x16x32_f16 per fragment pair
#define GH_LD 40   // 32 halfs + 8 pad
// the fp32 kernel k_gemm_nt<128,64> on the tiles of nd_gemm_plan (nd_gemm_f32.hip)
hipError_t nd_launch_gemm_nt_128x64(const float* x, const float* w, const float* bias, const float* res, float* out, int M, int K, int N,
                                    int act, int n_full, int split, float* part, unsigned grid, hipStream_t st);

// ---- attention core, d = 64: one launcher per form, each dispatching on NF = ceil(N / 16) key fragments ----
#define AT_MAXF 16  // up to 256 keys
hipError_t nd_launch_attention_ring(const float* qkv, float* out, int B, int N, int heads, int split_out, hipStream_t st);   // nd_attention.hip
hipError_t nd_launch_attention_b9(const void* att, float* out, int B, int N, int heads, int split_out, hipStream_t st);      // nd_attention_b9.hip
hipError_t nd_launch_attention_h(const float* qkv, float* out, int B, int N, int heads, hipStream_t st);                     // nd_attention_h.hip

// CALL(NF) for nf = 1 .. AT_MAXF as a compile-time constant; no case for any other nf
#define ND_DISPATCH_NF(nf, CALL)                                                                                                 \
    switch (nf) {                                                                                                                \
        case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break;                    \
        case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break;                    \
        case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;                  \
        case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; case 16: CALL(16); break;                  \
    }

// CALL(VPL) for the smallest VPL of {1, 2, 3, 4, 8} float4 per lane that holds vpl = ceil(dim / 256) (the LayerNorm kernels, one wave per row)
#define ND_DISPATCH_VPL(vpl, CALL)                                                                                               \
    do {                                                                                                                         \
        if ((vpl) <= 1) CALL(1); else if ((vpl) <= 2) CALL(2); else if ((vpl) <= 3) CALL(3); else if ((vpl) <= 4) CALL(4); else CALL(8); \
    } while (0)
