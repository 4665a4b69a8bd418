// nd_frag.hpp -- the operand layouts of the weight-streaming GEMMs (gfx950 / CDNA4 only): where an element lives, how a lane loads it.
//
// Skinny-M weight-streaming GEMM building blocks.  Every Linear on the sampling path has a small
// row count M (B*mc images, 32 at the headline config) against 4096..150528-wide weights, so the
// kernels are bound by streaming W once from HBM; the f32-input MFMA (v_mfma_f32_16x16x4_f32, exact
// f32) keeps the arithmetic off the VALU and just keeps up with the stream at M = 32.
//
// DATA LAYOUT ("frag16" packing).  Both GEMM operands are K-contiguous matrices A[R][K].  They are
// stored as 16-row x 16-column blocks of 1 KiB, block (r/16, k/16) at float offset
// ((r/16)*(K/16) + k/16)*256, and inside a block element (r, k) at ((r%16) + 16*((k%16)/4))*4 + k%4:
// exactly the order in which the 64 lanes of a wave consume it (lane l = row l&15, k-quad l>>4), so
// every wave-level load is one fully coalesced 1 KiB read and a workgroup streams one contiguous
// region.  Weights are packed once at load time; activations are written packed by the producing
// kernel's epilogue.  Measured on MI355X (tools/ubench_skinny.hip, 5 members x 67 MB): row-major
// operands 2.5 TB/s, packed 3.9 TB/s, packed + nontemporal W loads 4.2 TB/s (plain read: 5.4-6.0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nd_math.hpp"      // f32x4, f16x8

// float offset of element (r, k) of a frag16-packed matrix with nch = K/16 chunks per row
__host__ __device__ __forceinline__ size_t nd_pk(int r, int k, int nch) {
    return ((size_t)(r >> 4) * nch + (k >> 4)) * 256 + (size_t)(((r & 15) + 16 * ((k & 15) >> 2)) * 4 + (k & 3));
}
static inline size_t nd_packed_floats(int R, int K) { return (size_t)((R + 15) / 16) * 16 * (size_t)K; }

// HALF-PRECISION OPERANDS ("frag32h", the fp16 mode).  Same idea with 16-row x 32-column blocks of fp16, again 1 KiB:
// block (r/16, k/32) at BYTE offset ((r/16)*(K/32) + k/32)*1024, element (r, k) inside it at half index
// ((r%16) + 16*((k%32)/8))*8 + k%8 -- lane l of a wave holds the 8 halfs k = 8*(l>>4)..+7 of row l&15, the operand
// shape of v_mfma_f32_16x16x32_f16.  A block is 256 float-sized words like a frag16 block, so the streaming kernels
// address both forms identically with nch = K/32 instead of K/16.  Products are exact, accumulation is fp32.
__host__ __device__ __forceinline__ size_t nd_pkh(int r, int k, int nch32) {   // half index
    return ((size_t)(r >> 4) * nch32 + (k >> 5)) * 512 + (size_t)(((r & 15) + 16 * ((k & 31) >> 3)) * 8 + (k & 7));
}
static inline size_t nd_packed_bytes_dt(int R, int K, int half) {
    return (size_t)((R + 15) / 16) * 16 * (size_t)K * (half ? 2 : 4);
}

__device__ __forceinline__ f16x8 nd_as_h8(const float4& v) {   // the 16 bytes of a lane's operand, viewed as 8 halfs
    return __builtin_bit_cast(f16x8, v);
}

// 16-byte load from GLOBAL memory (address space 1: a pointer read out of a descriptor table is generic to the compiler
// and would become flat_load, which also counts on lgkmcnt).  NT = nontemporal (streamed once).
typedef __attribute__((address_space(1))) const f32x4 nd_gf4;
template <bool NT>
__device__ __forceinline__ float4 nd_ld16(const float* p) {
    const nd_gf4* g = (const nd_gf4*)p;
    const f32x4 v = NT ? __builtin_nontemporal_load(g) : *g;
    return make_float4(v[0], v[1], v[2], v[3]);
}

// scalar load from GLOBAL memory through a pointer the compiler only knows as generic (it came out of a descriptor table):
// a pending flat_load cannot be counted (it may be LDS or global), so every later wait would become vmcnt(0) lgkmcnt(0)
__device__ __forceinline__ float nd_ldg(const float* p) {
    return *(const __attribute__((address_space(1))) float*)p;
}

// struct copy out of the constant address space (scalar loads when the address is wave-uniform), word by word: the implicit copy
// constructor cannot bind an address-space-qualified source
template <typename T>
__device__ __forceinline__ T nd_ldc(const __attribute__((address_space(4))) void* p) {
    static_assert(sizeof(T) % 4 == 0, "word-sized structs only");
    T out;
    const __attribute__((address_space(4))) uint32_t* w = (const __attribute__((address_space(4))) uint32_t*)p;
    uint32_t* o = reinterpret_cast<uint32_t*>(&out);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) o[i] = w[i];
    return out;
}

// row-major fp32 [R, K] <-> frag16 (half = 0) / frag32h (half = 1, round to nearest even) image; csrc/nd_pack.hip.  The caller checks
// the launch (hipGetLastError).
void nd_launch_pack(const float* src, void* dst, int R, int K, int half, hipStream_t st);
void nd_launch_unpack(const void* src, float* dst, int R, int K, int half, hipStream_t st);
