// What the target-network files (target_ops.hip, tnet_patch.hip, tnet_msa.hip, tnet_head.hip, tnet_wgrad.hip) share.  Internal: not part of
// the C ABI.
#pragma once

#include "ghn3_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// wave-wide (64 lanes) butterfly reductions: every lane ends with the result
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline int wave_isum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- split-bf16 products on v_mfma_f32_16x16x32_bf16 (target_ops.hip, tnet_patch.hip) -------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
constexpr int KC = 32;       // reduction chunk = one v_mfma_f32_16x16x32_bf16 k-step
constexpr int LDK = 40;      // LDS row pitch in 16-bit elements (80 bytes: 16-byte aligned fragments)

// two values at once on the hardware converter (v_cvt_pk_bf16_f32, round to nearest even as bf16_rn): low half = a
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned bf16_pk(float a, float b) {
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ unsigned short bf16_rn(float v) { return (unsigned short)bf16_pk(v, v); }
// v = p[0] + p[1] (+ p[2]) in bf16 pieces: 16 (24) bits of mantissa.  With S = 3 pieces and the six products
// 11 + 12 + 21 + 22 + 13 + 31 the matrix-core product carries fp32's own rounding (~1e-7); S = 2 (hi.hi + lo.hi + hi.lo) ~1e-5.
template <int S>
__device__ __forceinline__ void splitS(float v, unsigned short* base, int idx, int stride) {
    float r = v;
#pragma unroll
    for (int q = 0; q < S; ++q) {
        const unsigned short h = bf16_rn(r);
        base[q * stride + idx] = h;
        r -= __uint_as_float((unsigned)h << 16);
    }
}
// acc[e] += sum_k A[lane & 15][k] B[4 (lane >> 4) + e][k]   (B fragment first: a lane owns 4 consecutive columns of a row)
__device__ __forceinline__ f32x4 mfma_bt(u16x8 b, u16x8 a, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b), __builtin_bit_cast(bf16x8, a), c, 0, 0, 0);
}
__device__ __forceinline__ u16x8 frag(const unsigned short* base, int row, int kc) {
    return *reinterpret_cast<const u16x8*>(base + row * LDK + 8 * kc);
}

template <int S>
__device__ __forceinline__ f32x4 mma_terms(const u16x8 (&a)[S], const u16x8 (&b)[S], f32x4 acc) {
    if (S == 3) { acc = mfma_bt(b[2], a[0], acc); acc = mfma_bt(b[0], a[2], acc); acc = mfma_bt(b[1], a[1], acc); }   // smallest first
    acc = mfma_bt(b[1], a[0], acc);
    acc = mfma_bt(b[0], a[1], acc);
    acc = mfma_bt(b[0], a[0], acc);
    return acc;
}

// scratch sections start on multiples of 64 floats
inline int64_t al(int64_t v) { return (v + 63) & ~(int64_t)63; }

#define TNET_LAUNCH_CHECK(what) { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { ghn3_set_error(what ": %s", hipGetErrorString(e_)); return GHN3_E_HIP; } }

// Raises a kernel's dynamic-LDS limit to `bytes`, once per kernel and process (keyed by the function's address: every
// instantiation of a kernel template has the same pointer TYPE).  Nothing to do at or below the default 48 KB.
template <typename K> int tnet_raise_lds(K kernel, size_t bytes) {
    static const void* done[32];
    static int n_done = 0;
    const void* key = (const void*)kernel;
    if (bytes <= 48 * 1024) return GHN3_OK;
    for (int i = 0; i < n_done; ++i)
        if (done[i] == key) return GHN3_OK;
    hipError_t e = hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) { ghn3_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return GHN3_E_HIP; }
    if (n_done < 32) done[n_done++] = key;
    return GHN3_OK;
}

// ---- tnet_wgrad.hip: the weight gradients of the linear layers ----------------------------------------------------------
// dW [Nout][K] (+ db [Nout] when bias) = G^T X over `rows` rows, G [rows][Nout], X [rows][K], as one product per chunk of
// tnet_wg_chunks(rows) row chunks.  part != null: the products go to part [chunk][Nout][K + bias] for tnet_reduce_launch;
// part == null (one chunk only): the product is the gradient and is written to w (and b).
struct TnetWgProb {
    const float* G; const float* X;
    float* part; float* w; float* b;
    int rows, Nout, K, bias;
};
constexpr int TNET_WG_MAX = 4;
int tnet_wg_chunks(int rows);
int64_t tnet_wg_part_floats(int rows, int Nout, int K);        // al(chunks Nout (K + 1)): a bias column is always counted
int tnet_wgrad_launch(const TnetWgProb* probs, int n, hipStream_t s);   // n <= TNET_WG_MAX, one launch

// out = sum over parts of part [parts][M], in part order.  ln == 0: element e = n ld + k -> w[n K + k] (k < K) or b[n]
// (k == K; b may be null); ln != 0: M = 2 K, element e < K -> w[e] (gamma), else b[e - K] (beta).
struct TnetRedProb { const float* part; float* w; float* b; int parts, M, ld, K, ln; };
constexpr int TNET_RED_MAX = 6;
int tnet_reduce_launch(const TnetRedProb* probs, int n, hipStream_t s); // n <= TNET_RED_MAX, one launch
// the reduction of a TnetWgProb's partials into its w (and b)
inline TnetRedProb tnet_wg_reduce(const TnetWgProb& q) {
    const int ld = q.K + q.bias;
    return TnetRedProb{q.part, q.w, q.bias ? q.b : nullptr, tnet_wg_chunks(q.rows), q.Nout * ld, ld, q.K, 0};
}
