// What the target-network files (target_ops.hip, tnet_msa.hip, tnet_head.hip, tnet_wgrad.hip) share.  Internal: not part of
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
