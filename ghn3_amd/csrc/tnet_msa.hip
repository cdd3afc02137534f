// Target-network layers: the `msa` op of the DeepNets-1M search space -- the pre-LN transformer layer of the ViT-style networks
// (ghn3/graphormer.py:144-248 with edge_dim = 0, built at ops.py:302; ghn3_amd.ops._TransformerLayer) -- forward and backward:
//
//     t  = tokens(x)                                                  (B, N = H W, C), x NCHW or NHWC
//     y1 = t + Wo attn(LN1(t) Wqkv^T [+ bqkv]) + bo
//     y  = y1 + W2 gelu_erf(W1 LN2(y1) + b1) + b2
//     out = y[::s, ::s]                                               NHWC (B, Ho, Wo, C)
//
//   forward   msa_ln_qkv      a workgroup owns RB token rows: x read as it is (NCHW rows gathered through LDS), LN1 row
//                             statistics, the normalised rows as the A operand of the QKV product; writes qkv [B N][3 C] -- the
//                             layout ghn3_attn_fwd reads -- and fills the per-sequence token counts the attention reads;
//             ghn3_attn_fwd   (attention.hip) no bias, P saved only when the backward will run;
//             msa_post        the KEPT rows only (h % s == 0, w % s == 0): out-projection + bo + residual, LN2, FF1 + b1,
//                             GELU (erf), FF2 + b2 + residual; every intermediate stays in LDS; saves y1, the LN2 statistics
//                             and the pre-GELU values for the backward.
//   backward  msa_post_bwd    dout -> dh = (dout W2) gelu'(pre) -> da2 = dh W1 -> LN2 backward -> dy1 (+ dout) -> dO = dy1 Wo
//                             (dropped rows: zero); LN2 parameter partials per workgroup;
//             ghn3_attn_bwd   -> dqkv;
//             msa_qkv_bwd     da1 = dqkv Wqkv -> LN1 backward -> + dy1 -> dx in x's layout; LN1 parameter partials;
//             tnet_wgrad      (tnet_wgrad.hip) the four weight (+ bias) gradients dW = G^T X as fixed row-chunk partial
//                             products;
//             tnet_reduce     (tnet_wgrad.hip) fixed-order sums of every partial, the LayerNorm ones included -> dense
//                             gradients.
//
// Every product runs on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate; no 16-bit operands: the target networks
// and their stock path are fp32).  Each lane feeds one float4 of A and of B per four MFMAs: instruction j of a 16-wide k step
// takes k = k0 + 4 (lane >> 4) + j for both operands, a permutation of the summation order only.  No float atomics anywhere:
// reruns are bit-identical.  Limits (host-checked): C % 4 == 0, C <= 256, d = C / heads <= 32, N <= 4096, hidden % 4 == 0 and
// <= 1024, element counts < 2^31.

#include <algorithm>
#include "tnet_common.h"

namespace {

constexpr int NT = 256;                     // threads per workgroup (4 waves)
constexpr int MAX_LDS = 160 * 1024;

struct MsaDims {
    int B, H, W, C, heads, hidden, stride, Ho, Wo, layout;
    float eps;
    int N, R, Kr;                           // tokens per sequence, token rows B N, kept rows B Ho Wo
};

__host__ __device__ inline int r16(int v) { return (v + 15) & ~15; }

// token row of kept row kr
__device__ inline int kept_row(const MsaDims& d, int kr) {
    const int hw = d.Ho * d.Wo, b = kr / hw, p = kr - b * hw, ho = p / d.Wo, wo = p - ho * d.Wo;
    return b * d.N + ho * d.stride * d.W + wo * d.stride;
}

// offset of element (token row r, channel c) of an activation in the input layout
__device__ inline size_t x_off(const MsaDims& d, int r, int c) {
    if (d.layout) return (size_t)r * d.C + c;
    const int b = r / d.N, n = r - b * d.N;
    return ((size_t)b * d.C + c) * d.N + n;
}

__device__ inline float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
__device__ inline float gelu_erf_grad(float v) {
    return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * expf(-0.5f * v * v);
}

// Y [16 RT rows][Nout] = A op(W) on the fp32 matrix cores, the workgroup's waves taking the 16-wide column tiles in turn.
//   A: LDS, 16 RT rows of lda floats, columns K .. r16(K) zero (and every row finite);
//   WT = false: W [Nout][K] row-major, Y = A W^T (nn.Linear);   WT = true: W [K][Nout] row-major, Y = A W.
// epi(row, col, value) is called once per element with col < Nout (16 consecutive columns per quarter-wave).
template <int RT, bool WT, class Epi>
__device__ inline void rows_gemm(const float* A, int lda, const float* __restrict__ W, int K, int Nout, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int nct = (Nout + 15) >> 4;
    for (int ct = wave; ct < nct; ct += NT / 64) {
        const int n = ct * 16 + i;
        const bool nok = n < Nout;
        const int nc = nok ? n : Nout - 1;
        f32x4 acc[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < K; k0 += 16) {
            const int k = k0 + 4 * q;
            const bool ok = nok && k < K;                 // (K % 4 == 0: a float4 is wholly inside or outside)
            const int kc = k < K ? k : 0;
            f32x4 b;
            if (!WT) {
                b = *reinterpret_cast<const f32x4*>(W + (size_t)nc * K + kc);
            } else {
                const float* p = W + (size_t)kc * Nout + nc;
                b = f32x4{p[0], p[Nout], p[2 * (size_t)Nout], p[3 * (size_t)Nout]};
            }
            if (!ok) b = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(A + (r * 16 + i) * lda + k);
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc[r], 0, 0, 0);
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc[r], 0, 0, 0);
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc[r], 0, 0, 0);
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc[r], 0, 0, 0);
            }
        }
        if (nok) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int g = 0; g < 4; ++g) epi(r * 16 + 4 * q + g, n, acc[r][g]);     // C/D: row 4 (lane >> 4) + reg, col lane & 15
        }
    }
}

// zero columns [c0, c1) of RB rows of an LDS image
__device__ inline void zero_cols(float* A, int lda, int rows, int c0, int c1) {
    const int w = c1 - c0;
    for (int e = threadIdx.x; e < rows * w; e += NT) A[(e / w) * lda + c0 + e % w] = 0.f;
}

// RB rows of a row-major [rows][ld] global matrix (row index from rowmap) into LDS; rows >= count are zero
template <int RB, class RowMap>
__device__ inline void load_rows(float* A, int lda, const float* __restrict__ src, int ld, int cols, int first, int count,
                                 RowMap rowmap) {
    const int c4 = cols >> 2;
    for (int e = threadIdx.x; e < RB * c4; e += NT) {
        const int row = e / c4, c = (e - row * c4) * 4, r = first + row;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < count) v = *reinterpret_cast<const f32x4*>(src + (size_t)rowmap(r) * ld + c);
        *reinterpret_cast<f32x4*>(A + row * lda + c) = v;
    }
}

// token rows [first, first + RB) of x (input layout) into LDS [RB][lda] (kept = true: rows are kept-row indices)
template <int RB>
__device__ inline void load_x_rows(float* A, int lda, const float* __restrict__ x, const MsaDims& d, int first, int count,
                                   bool kept) {
    if (d.layout) {
        const int c4 = d.C >> 2;
        for (int e = threadIdx.x; e < RB * c4; e += NT) {
            const int row = e / c4, c = (e - row * c4) * 4, r = first + row;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r < count) v = *reinterpret_cast<const f32x4*>(x + (size_t)(kept ? kept_row(d, r) : r) * d.C + c);
            *reinterpret_cast<f32x4*>(A + row * lda + c) = v;
        }
    } else {
        // NCHW: consecutive threads take consecutive tokens of one channel (coalesced within a sequence)
        for (int e = threadIdx.x; e < RB * d.C; e += NT) {
            const int c = e / RB, row = e - c * RB, r = first + row;
            A[row * lda + c] = r < count ? x[x_off(d, kept ? kept_row(d, r) : r, c)] : 0.f;
        }
    }
}

// LayerNorm of RB LDS rows in place (wave per row): two-pass biased variance as torch; stats [row][2] = mean, rstd
template <int RB>
__device__ inline void ln_rows(float* A, int lda, int C, float eps, const float* __restrict__ g, const float* __restrict__ be,
                               int first, int count, float* __restrict__ stats, float* __restrict__ save_in) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = wave; row < RB; row += NT / 64) {
        const int r = first + row;
        if (r >= count) continue;                                   // (wave-uniform; the row stays zero)
        float* a = A + row * lda;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += a[c];
        const float mean = wave_sum(s) / (float)C;
        float v = 0.f;
        for (int c = lane; c < C; c += 64) { const float t = a[c] - mean; v += t * t; }
        const float rstd = 1.f / sqrtf(wave_sum(v) / (float)C + eps);
        for (int c = lane; c < C; c += 64) {
            if (save_in) save_in[(size_t)r * C + c] = a[c];
            a[c] = (a[c] - mean) * rstd * g[c] + be[c];
        }
        if (stats && lane == 0) { stats[2 * (size_t)r] = mean; stats[2 * (size_t)r + 1] = rstd; }
    }
}

// ------------------------------------------------------------------------------------------------ forward
template <int RB>
__global__ __launch_bounds__(NT) void msa_ln_qkv_kernel(MsaDims d, const float* __restrict__ x, ghn3_msa_params p,
                                                          float* __restrict__ qkv, float* __restrict__ stats1, int* __restrict__ n_nodes) {
    extern __shared__ float lds[];
    const int ldc = r16(d.C) + 4, first = blockIdx.x * RB;
    if (blockIdx.x == 0)
        for (int b = threadIdx.x; b < d.B; b += NT) n_nodes[b] = d.N;
    load_x_rows<RB>(lds, ldc, x, d, first, d.R, false);
    zero_cols(lds, ldc, RB, d.C, r16(d.C));
    __syncthreads();
    ln_rows<RB>(lds, ldc, d.C, d.eps, p.ln1_w, p.ln1_b, first, d.R, stats1, nullptr);
    __syncthreads();
    const int C3 = 3 * d.C;
    const float* bq = p.b_qkv;
    rows_gemm<RB / 16, false>(lds, ldc, p.w_qkv, d.C, C3, [&](int row, int n, float v) {
        const int r = first + row;
        if (r < d.R) qkv[(size_t)r * C3 + n] = v + (bq ? bq[n] : 0.f);
    });
}

// LDS: A [RB][ldc] (O rows, then LN2(y1)), Y [RB][ldc] (y1), H [RB][ldh] (gelu(h))
template <int RB>
__global__ __launch_bounds__(NT) void msa_post_kernel(MsaDims d, const float* __restrict__ x, const float* __restrict__ O,
                                                        ghn3_msa_params p, float* __restrict__ out, float* __restrict__ y1s,
                                                        float* __restrict__ stats2, float* __restrict__ pre) {
    extern __shared__ float lds[];
    const int C = d.C, hid = d.hidden, ldc = r16(C) + 4, ldh = r16(hid) + 4, first = blockIdx.x * RB;
    float* A = lds;
    float* Y = A + RB * ldc;
    float* Hs = Y + RB * ldc;
    load_rows<RB>(A, ldc, O, C, C, first, d.Kr, [&](int r) { return kept_row(d, r); });
    load_x_rows<RB>(Y, ldc, x, d, first, d.Kr, true);
    zero_cols(A, ldc, RB, C, r16(C));
    zero_cols(Hs, ldh, RB, hid, r16(hid));
    __syncthreads();
    rows_gemm<RB / 16, false>(A, ldc, p.w_o, C, C, [&](int row, int n, float v) {
        if (first + row < d.Kr) Y[row * ldc + n] += v + p.b_o[n];
    });
    __syncthreads();
    // LN2(y1) into A (y1 kept in Y for the second residual)
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int row = wave; row < RB; row += NT / 64) {
            const int r = first + row;
            if (r >= d.Kr) continue;
            const float* y = Y + row * ldc;
            float s = 0.f;
            for (int c = lane; c < C; c += 64) s += y[c];
            const float mean = wave_sum(s) / (float)C;
            float v = 0.f;
            for (int c = lane; c < C; c += 64) { const float t = y[c] - mean; v += t * t; }
            const float rstd = 1.f / sqrtf(wave_sum(v) / (float)C + d.eps);
            for (int c = lane; c < C; c += 64) {
                A[row * ldc + c] = (y[c] - mean) * rstd * p.ln2_w[c] + p.ln2_b[c];
                if (y1s) y1s[(size_t)r * C + c] = y[c];
            }
            if (stats2 && lane == 0) { stats2[2 * (size_t)r] = mean; stats2[2 * (size_t)r + 1] = rstd; }
        }
    }
    __syncthreads();
    rows_gemm<RB / 16, false>(A, ldc, p.w1, C, hid, [&](int row, int n, float v) {
        const int r = first + row;
        float h = 0.f;
        if (r < d.Kr) {
            h = v + p.b1[n];
            if (pre) pre[(size_t)r * hid + n] = h;
        }
        Hs[row * ldh + n] = gelu_erf(h);
    });
    __syncthreads();
    rows_gemm<RB / 16, false>(Hs, ldh, p.w2, hid, C, [&](int row, int n, float v) {
        const int r = first + row;
        if (r < d.Kr) out[(size_t)r * C + n] = Y[row * ldc + n] + v + p.b2[n];
    });
}

// ------------------------------------------------------------------------------------------------ backward
// LDS: G [RB][ldc] (dout, then da2 . xhat2), Hs [RB][ldm] (dh, then dy1), D [RB][ldc] (da2)
template <int RB>
__global__ __launch_bounds__(NT) void msa_post_bwd_kernel(MsaDims d, const float* __restrict__ dout, ghn3_msa_params p,
                                                            const float* __restrict__ y1s, const float* __restrict__ stats2,
                                                            const float* __restrict__ pre, float* __restrict__ dh_s,
                                                            float* __restrict__ gact, float* __restrict__ a2s,
                                                            float* __restrict__ dy1, float* __restrict__ dO,
                                                            float* __restrict__ ln2_part) {
    extern __shared__ float lds[];
    const int C = d.C, hid = d.hidden, ldc = r16(C) + 4, ldm = max(r16(hid), r16(C)) + 4, first = blockIdx.x * RB;
    float* G = lds;
    float* Hs = G + RB * ldc;
    float* D = Hs + RB * ldm;
    load_rows<RB>(G, ldc, dout, C, C, first, d.Kr, [](int r) { return r; });
    zero_cols(G, ldc, RB, C, r16(C));
    zero_cols(Hs, ldm, RB, hid, ldm - 4);
    __syncthreads();
    rows_gemm<RB / 16, true>(G, ldc, p.w2, C, hid, [&](int row, int n, float v) {
        const int r = first + row;
        float g = 0.f;
        if (r < d.Kr) {
            const float h = pre[(size_t)r * hid + n];
            g = v * gelu_erf_grad(h);
            dh_s[(size_t)r * hid + n] = g;
            gact[(size_t)r * hid + n] = gelu_erf(h);
        }
        Hs[row * ldm + n] = g;
    });
    __syncthreads();
    rows_gemm<RB / 16, true>(Hs, ldm, p.w1, hid, C, [&](int row, int n, float v) { D[row * ldc + n] = v; });
    __syncthreads();
    // LN2 backward (wave per row): dy1 = dout + rstd (dxh - mean(dxh) - xhat mean(dxh xhat)), dxh = da2 . gamma2
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int row = wave; row < RB; row += NT / 64) {
            const int r = first + row;
            float* hrow = Hs + row * ldm;
            if (r >= d.Kr) {
                for (int c = lane; c < ldm - 4; c += 64) hrow[c] = 0.f;
                continue;
            }
            const float mean = stats2[2 * (size_t)r], rstd = stats2[2 * (size_t)r + 1];
            const float* y = y1s + (size_t)r * C;
            float s1 = 0.f, s2 = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float xh = (y[c] - mean) * rstd, dxh = D[row * ldc + c] * p.ln2_w[c];
                s1 += dxh;
                s2 += dxh * xh;
            }
            s1 = wave_sum(s1) / (float)C;
            s2 = wave_sum(s2) / (float)C;
            const int tr = kept_row(d, r);
            for (int c = lane; c < C; c += 64) {
                const float xh = (y[c] - mean) * rstd, da = D[row * ldc + c], dxh = da * p.ln2_w[c];
                const float g = G[row * ldc + c] + rstd * (dxh - s1 - xh * s2);
                G[row * ldc + c] = da * xh;
                a2s[(size_t)r * C + c] = xh * p.ln2_w[c] + p.ln2_b[c];
                dy1[(size_t)tr * C + c] = g;
                hrow[c] = g;
            }
            for (int c = C + lane; c < ldm - 4; c += 64) hrow[c] = 0.f;
        }
    }
    __syncthreads();
    // LN2 parameter partials of this workgroup (rows in order) and dO = dy1 Wo
    for (int c = threadIdx.x; c < C; c += NT) {
        float sg = 0.f, sb = 0.f;
        for (int row = 0; row < RB; ++row) { sg += G[row * ldc + c]; sb += D[row * ldc + c]; }
        ln2_part[(size_t)blockIdx.x * 2 * C + c] = sg;
        ln2_part[(size_t)blockIdx.x * 2 * C + C + c] = sb;
    }
    rows_gemm<RB / 16, true>(Hs, ldm, p.w_o, C, C, [&](int row, int n, float v) {
        const int r = first + row;
        if (r < d.Kr) dO[(size_t)kept_row(d, r) * C + n] = v;
    });
}

// LDS: Q [RB][ld3] (dqkv rows; then columns [0, C) x -> dx and [C, 2C) da1 . xhat1), A [RB][ldc] (da1)
template <int RB>
__global__ __launch_bounds__(NT) void msa_qkv_bwd_kernel(MsaDims d, const float* __restrict__ x, ghn3_msa_params p,
                                                           const float* __restrict__ dqkv, const float* __restrict__ stats1,
                                                           const float* __restrict__ dy1, float* __restrict__ a1s,
                                                           float* __restrict__ dx, float* __restrict__ ln1_part) {
    extern __shared__ float lds[];
    const int C = d.C, C3 = 3 * C, ldc = r16(C) + 4, ld3 = r16(C3) + 4, first = blockIdx.x * RB;
    float* Q = lds;
    float* A = Q + RB * ld3;
    load_rows<RB>(Q, ld3, dqkv, C3, C3, first, d.R, [](int r) { return r; });
    zero_cols(Q, ld3, RB, C3, r16(C3));
    __syncthreads();
    rows_gemm<RB / 16, true>(Q, ld3, p.w_qkv, C3, C, [&](int row, int n, float v) { A[row * ldc + n] = v; });
    __syncthreads();
    load_x_rows<RB>(Q, ld3, x, d, first, d.R, false);
    __syncthreads();
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int row = wave; row < RB; row += NT / 64) {
            const int r = first + row;
            float* q = Q + row * ld3;
            if (r >= d.R) {
                for (int c = lane; c < C; c += 64) q[C + c] = 0.f;
                continue;
            }
            const float mean = stats1[2 * (size_t)r], rstd = stats1[2 * (size_t)r + 1];
            float s1 = 0.f, s2 = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float xh = (q[c] - mean) * rstd, dxh = A[row * ldc + c] * p.ln1_w[c];
                s1 += dxh;
                s2 += dxh * xh;
            }
            s1 = wave_sum(s1) / (float)C;
            s2 = wave_sum(s2) / (float)C;
            for (int c = lane; c < C; c += 64) {
                const float xh = (q[c] - mean) * rstd, da = A[row * ldc + c], dxh = da * p.ln1_w[c];
                a1s[(size_t)r * C + c] = xh * p.ln1_w[c] + p.ln1_b[c];
                q[c] = dy1[(size_t)r * C + c] + rstd * (dxh - s1 - xh * s2);
                q[C + c] = da * xh;
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += NT) {
        float sg = 0.f, sb = 0.f;
        for (int row = 0; row < RB; ++row) { sg += Q[row * ld3 + C + c]; sb += A[row * ldc + c]; }
        ln1_part[(size_t)blockIdx.x * 2 * C + c] = sg;
        ln1_part[(size_t)blockIdx.x * 2 * C + C + c] = sb;
    }
    // dx in x's layout (NCHW: consecutive threads write consecutive tokens of a channel)
    if (d.layout) {
        const int c4 = C >> 2;
        for (int e = threadIdx.x; e < RB * c4; e += NT) {
            const int row = e / c4, c = (e - row * c4) * 4, r = first + row;
            if (r < d.R) *reinterpret_cast<f32x4*>(dx + (size_t)r * C + c) = *reinterpret_cast<const f32x4*>(Q + row * ld3 + c);
        }
    } else {
        for (int e = threadIdx.x; e < RB * C; e += NT) {
            const int c = e / RB, row = e - c * RB, r = first + row;
            if (r < d.R) dx[x_off(d, r, c)] = Q[row * ld3 + c];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
int check(const ghn3_msa_desc* g, MsaDims* out) {
    if (!g) { ghn3_set_error("msa: null descriptor"); return GHN3_E_ARG; }
    const ghn3_msa_desc& s = *g;
    if (s.B <= 0 || s.H <= 0 || s.W <= 0 || s.C <= 0 || s.heads <= 0 || s.hidden <= 0 || s.stride <= 0 || s.Ho <= 0 || s.Wo <= 0) {
        ghn3_set_error("msa: non-positive size in the descriptor");
        return GHN3_E_ARG;
    }
    if (s.layout != 0 && s.layout != 1) { ghn3_set_error("msa: layout %d is neither 0 (NCHW) nor 1 (NHWC)", s.layout); return GHN3_E_ARG; }
    if (s.Ho != (s.H - 1) / s.stride + 1 || s.Wo != (s.W - 1) / s.stride + 1) {
        ghn3_set_error("msa: output grid %d x %d does not match H, W, stride", s.Ho, s.Wo);
        return GHN3_E_ARG;
    }
    const int64_t N = (int64_t)s.H * s.W;
    if (s.C % 4 || s.C > 256 || s.C % s.heads || s.C / s.heads > 32) {
        ghn3_set_error("msa: needs C %% 4 == 0, C <= 256, C %% heads == 0 and head dim <= 32 (C %d, heads %d)", s.C, s.heads);
        return GHN3_E_LIMIT;
    }
    if (N > 4096) { ghn3_set_error("msa: %lld tokens per sequence (limit 4096)", (long long)N); return GHN3_E_LIMIT; }
    if (s.hidden % 4 || s.hidden > 1024) { ghn3_set_error("msa: hidden %d not a multiple of 4 or above 1024", s.hidden); return GHN3_E_LIMIT; }
    const int64_t R = s.B * N;
    if (R * 3 * s.C >= (1ll << 31) || R * s.hidden >= (1ll << 31) || (int64_t)s.B * s.heads * N * N >= (1ll << 31)) {
        ghn3_set_error("msa: tensors of 2^31 elements or more are not supported");
        return GHN3_E_LIMIT;
    }
    if (out) {
        *out = MsaDims{s.B, s.H, s.W, s.C, s.heads, s.hidden, s.stride, s.Ho, s.Wo, s.layout, s.eps, (int)N, (int)R,
                       s.B * s.Ho * s.Wo};
    }
    return GHN3_OK;
}

// the row blocks: 32 rows unless the widest kernel of the pass needs more LDS than a CU has
int lds_post(int RB, const MsaDims& d) { return RB * (2 * (r16(d.C) + 4) + r16(d.hidden) + 4) * 4; }
int lds_post_bwd(int RB, const MsaDims& d) { return RB * (2 * (r16(d.C) + 4) + std::max(r16(d.hidden), r16(d.C)) + 4) * 4; }
int lds_qkv_bwd(int RB, const MsaDims& d) { return RB * (r16(3 * d.C) + 4 + r16(d.C) + 4) * 4; }
int pick_rb(const MsaDims& d) {
    const int need = std::max(std::max(lds_post(32, d), lds_post_bwd(32, d)), lds_qkv_bwd(32, d));
    return need <= MAX_LDS ? 32 : 16;
}

// forward scratch (kept for the backward): n_nodes | stats1 | qkv | O | y1 | stats2 | pre
struct FwdLayout { int64_t nn, stats1, qkv, O, y1, stats2, pre, total; };
FwdLayout fwd_layout(const MsaDims& d) {
    FwdLayout f;
    int64_t o = 0;
    f.nn = o; o += al(d.B);
    f.stats1 = o; o += al(2 * (int64_t)d.R);
    f.qkv = o; o += al(3 * (int64_t)d.R * d.C);
    f.O = o; o += al((int64_t)d.R * d.C);
    f.y1 = o; o += al((int64_t)d.Kr * d.C);
    f.stats2 = o; o += al(2 * (int64_t)d.Kr);
    f.pre = o; o += al((int64_t)d.Kr * d.hidden);
    f.total = o;
    return f;
}

// backward scratch: dO | dy1 | dqkv | a1 | dh | gact | a2 | ln2 parts | ln1 parts | weight-gradient parts (qkv, o, 1, 2)
struct BwdLayout { int64_t dO, dy1, dqkv, a1, dh, gact, a2, ln2, ln1, pq, po, p1, p2, total; };
BwdLayout bwd_layout(const MsaDims& d) {
    const int RB = pick_rb(d);
    BwdLayout b;
    int64_t o = 0;
    b.dO = o; o += al((int64_t)d.R * d.C);
    b.dy1 = o; o += al((int64_t)d.R * d.C);
    b.dqkv = o; o += al(3 * (int64_t)d.R * d.C);
    b.a1 = o; o += al((int64_t)d.R * d.C);
    b.dh = o; o += al((int64_t)d.Kr * d.hidden);
    b.gact = o; o += al((int64_t)d.Kr * d.hidden);
    b.a2 = o; o += al((int64_t)d.Kr * d.C);
    b.ln2 = o; o += al((int64_t)((d.Kr + RB - 1) / RB) * 2 * d.C);
    b.ln1 = o; o += al((int64_t)((d.R + RB - 1) / RB) * 2 * d.C);
    b.pq = o; o += tnet_wg_part_floats(d.R, 3 * d.C, d.C);
    b.po = o; o += tnet_wg_part_floats(d.R, d.C, d.C);
    b.p1 = o; o += tnet_wg_part_floats(d.Kr, d.hidden, d.C);
    b.p2 = o; o += tnet_wg_part_floats(d.Kr, d.C, d.hidden);
    b.total = o;
    return b;
}

template <int RB>
int fwd_rb(const MsaDims& d, const float* x, const ghn3_msa_params& p, float* out, float* scratch, float* P, hipStream_t s) {
    const FwdLayout f = fwd_layout(d);
    int* nn = reinterpret_cast<int*>(scratch + f.nn);
    const bool train = P != nullptr;
    int rc;
    size_t lds = (size_t)RB * (r16(d.C) + 4) * 4;
    if ((rc = tnet_raise_lds(msa_ln_qkv_kernel<RB>, MAX_LDS))) return rc;
    hipLaunchKernelGGL(msa_ln_qkv_kernel<RB>, dim3((d.R + RB - 1) / RB), dim3(NT), lds, s, d, x, p, scratch + f.qkv,
                       scratch + f.stats1, nn);
    TNET_LAUNCH_CHECK("msa ln_qkv");
    if ((rc = ghn3_attn_fwd(scratch + f.O, scratch + f.qkv, nullptr, P, nn, d.B, d.N, d.C, d.heads, s))) return rc;
    if ((rc = tnet_raise_lds(msa_post_kernel<RB>, MAX_LDS))) return rc;
    hipLaunchKernelGGL(msa_post_kernel<RB>, dim3((d.Kr + RB - 1) / RB), dim3(NT), (size_t)lds_post(RB, d), s, d, x,
                       (const float*)(scratch + f.O), p, out, train ? scratch + f.y1 : nullptr,
                       train ? scratch + f.stats2 : nullptr, train ? scratch + f.pre : nullptr);
    TNET_LAUNCH_CHECK("msa post");
    return GHN3_OK;
}

template <int RB>
int bwd_rb(const MsaDims& d, const float* dout, const float* x, const ghn3_msa_params& p, const float* fs, const float* P,
           float* dx, const ghn3_msa_grads& g, float* scratch, hipStream_t s) {
    const FwdLayout f = fwd_layout(d);
    const BwdLayout b = bwd_layout(d);
    const int* nn = reinterpret_cast<const int*>(fs + f.nn);
    int rc;
    if (d.Kr != d.R) {                           // (dropped rows: no gradient reaches them through y)
        hipError_t e = hipMemsetAsync(scratch + b.dO, 0, (size_t)(b.dy1 - b.dO + (int64_t)d.R * d.C) * sizeof(float), s);  // dO, dy1
        if (e != hipSuccess) { ghn3_set_error("msa bwd: hipMemsetAsync: %s", hipGetErrorString(e)); return GHN3_E_HIP; }
    }
    const int nb_post = (d.Kr + RB - 1) / RB, nb_rows = (d.R + RB - 1) / RB;
    if ((rc = tnet_raise_lds(msa_post_bwd_kernel<RB>, MAX_LDS))) return rc;
    hipLaunchKernelGGL(msa_post_bwd_kernel<RB>, dim3(nb_post), dim3(NT), (size_t)lds_post_bwd(RB, d), s, d, dout, p,
                       fs + f.y1, fs + f.stats2, fs + f.pre, scratch + b.dh, scratch + b.gact, scratch + b.a2, scratch + b.dy1,
                       scratch + b.dO, scratch + b.ln2);
    TNET_LAUNCH_CHECK("msa post bwd");
    if ((rc = ghn3_attn_bwd(scratch + b.dqkv, scratch + b.dO, fs + f.qkv, P, fs + f.O, nullptr, nullptr, nn, d.B, d.N, d.C,
                            d.heads, 0, s)))
        return rc;
    if ((rc = tnet_raise_lds(msa_qkv_bwd_kernel<RB>, MAX_LDS))) return rc;
    hipLaunchKernelGGL(msa_qkv_bwd_kernel<RB>, dim3(nb_rows), dim3(NT), (size_t)lds_qkv_bwd(RB, d), s, d, x, p,
                       (const float*)(scratch + b.dqkv), fs + f.stats1, (const float*)(scratch + b.dy1), scratch + b.a1, dx,
                       scratch + b.ln1);
    TNET_LAUNCH_CHECK("msa qkv bwd");
    // weight gradients: dWqkv = dqkv^T a1, dWo = dy1^T O (rows of all tokens; dropped ones are zero), dW1 = dh^T a2, dW2 = dout^T gelu
    const TnetWgProb wg[4] = {
        {scratch + b.dqkv, scratch + b.a1, scratch + b.pq, g.w_qkv, g.b_qkv, d.R, 3 * d.C, d.C, g.b_qkv != nullptr},
        {scratch + b.dy1, fs + f.O, scratch + b.po, g.w_o, g.b_o, d.R, d.C, d.C, 1},
        {scratch + b.dh, scratch + b.a2, scratch + b.p1, g.w1, g.b1, d.Kr, d.hidden, d.C, 1},
        {dout, scratch + b.gact, scratch + b.p2, g.w2, g.b2, d.Kr, d.C, d.hidden, 1},
    };
    if ((rc = tnet_wgrad_launch(wg, 4, s))) return rc;
    const TnetRedProb red[6] = {
        tnet_wg_reduce(wg[0]), tnet_wg_reduce(wg[1]), tnet_wg_reduce(wg[2]), tnet_wg_reduce(wg[3]),
        {scratch + b.ln1, g.ln1_w, g.ln1_b, nb_rows, 2 * d.C, d.C, d.C, 1},
        {scratch + b.ln2, g.ln2_w, g.ln2_b, nb_post, 2 * d.C, d.C, d.C, 1},
    };
    return tnet_reduce_launch(red, 6, s);
}

bool a16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// every pointer present; the ones read or written as float4 16-byte aligned
bool params_ok(const ghn3_msa_params* p, int has_qkv_bias) {
    return p && p->ln1_w && p->ln1_b && p->w_qkv && (!has_qkv_bias || p->b_qkv) && p->w_o && p->b_o && p->ln2_w && p->ln2_b &&
           p->w1 && p->b1 && p->w2 && p->b2 && a16(p->w_qkv) && a16(p->w_o) && a16(p->w1) && a16(p->w2);
}

}  // namespace

extern "C" int64_t ghn3_msa_scratch_floats(const ghn3_msa_desc* desc, int backward) {
    MsaDims d;
    const int rc = check(desc, &d);
    if (rc) return rc;
    return backward ? bwd_layout(d).total : fwd_layout(d).total;
}

extern "C" int ghn3_msa_fwd(const ghn3_msa_desc* desc, const float* x, const ghn3_msa_params* params, float* out, float* P,
                            float* scratch, void* stream) {
    MsaDims d;
    int rc = check(desc, &d);
    if (rc) return rc;
    if (!x || !out || !scratch || !params_ok(params, desc->has_qkv_bias) || !a16(x) || !a16(scratch)) {
        ghn3_set_error("msa fwd: null or misaligned pointer (x, scratch and the weight matrices need 16-byte alignment)");
        return GHN3_E_ARG;
    }
    ghn3_msa_params p = *params;
    if (!desc->has_qkv_bias) p.b_qkv = nullptr;
    hipStream_t s = (hipStream_t)stream;
    return pick_rb(d) == 32 ? fwd_rb<32>(d, x, p, out, scratch, P, s) : fwd_rb<16>(d, x, p, out, scratch, P, s);
}

extern "C" int ghn3_msa_bwd(const ghn3_msa_desc* desc, const float* dout, const float* x, const ghn3_msa_params* params,
                            const float* fwd_scratch, const float* P, float* dx, const ghn3_msa_grads* grads, float* scratch,
                            void* stream) {
    MsaDims d;
    int rc = check(desc, &d);
    if (rc) return rc;
    if (!dout || !x || !fwd_scratch || !P || !dx || !scratch || !grads || !params_ok(params, desc->has_qkv_bias) || !a16(dout) ||
        !a16(x) || !a16(fwd_scratch) || !a16(P) || !a16(dx) || !a16(scratch)) {
        ghn3_set_error("msa bwd: null or misaligned pointer");
        return GHN3_E_ARG;
    }
    const ghn3_msa_grads& g = *grads;
    if (!g.ln1_w || !g.ln1_b || !g.w_qkv || (desc->has_qkv_bias && !g.b_qkv) || !g.w_o || !g.b_o || !g.ln2_w || !g.ln2_b ||
        !g.w1 || !g.b1 || !g.w2 || !g.b2) {
        ghn3_set_error("msa bwd: null gradient pointer");
        return GHN3_E_ARG;
    }
    ghn3_msa_params p = *params;
    ghn3_msa_grads gg = g;
    if (!desc->has_qkv_bias) { p.b_qkv = nullptr; gg.b_qkv = nullptr; }
    hipStream_t s = (hipStream_t)stream;
    return pick_rb(d) == 32 ? bwd_rb<32>(d, dout, x, p, fwd_scratch, P, dx, gg, scratch, s)
                            : bwd_rb<16>(d, dout, x, p, fwd_scratch, P, dx, gg, scratch, s);
}

// ------------------------------------------------------------------------------------------------ lean attention
// ghn3_msa_lean_*: the same layer on the attention of tnet_attn.hip, which recomputes the probabilities in the backward from one
// float per query row (lse) instead of reading a saved P [B][heads][N][N].  Every other kernel runs as above, unchanged.
namespace {

// check() without its B heads N^2 term -- no tensor of that size exists here.  (Stated in full rather than shared, so that the
// saved-P entry points and their refusals stay as they are, text included.)
int check_lean(const ghn3_msa_desc* g, MsaDims* out) {
    if (!g) { ghn3_set_error("msa lean: null descriptor"); return GHN3_E_ARG; }
    const ghn3_msa_desc& s = *g;
    if (s.B <= 0 || s.H <= 0 || s.W <= 0 || s.C <= 0 || s.heads <= 0 || s.hidden <= 0 || s.stride <= 0 || s.Ho <= 0 || s.Wo <= 0) {
        ghn3_set_error("msa lean: non-positive size in the descriptor");
        return GHN3_E_ARG;
    }
    if (s.layout != 0 && s.layout != 1) { ghn3_set_error("msa lean: layout %d is neither 0 (NCHW) nor 1 (NHWC)", s.layout); return GHN3_E_ARG; }
    if (s.Ho != (s.H - 1) / s.stride + 1 || s.Wo != (s.W - 1) / s.stride + 1) {
        ghn3_set_error("msa lean: output grid %d x %d does not match H, W, stride", s.Ho, s.Wo);
        return GHN3_E_ARG;
    }
    const int64_t N = (int64_t)s.H * s.W;
    if (s.C % 4 || s.C > 256 || s.C % s.heads || s.C / s.heads > 32) {
        ghn3_set_error("msa lean: needs C %% 4 == 0, C <= 256, C %% heads == 0 and head dim <= 32 (C %d, heads %d)", s.C, s.heads);
        return GHN3_E_LIMIT;
    }
    if (N > 4096) { ghn3_set_error("msa lean: %lld tokens per sequence (limit 4096)", (long long)N); return GHN3_E_LIMIT; }
    if (s.hidden % 4 || s.hidden > 1024) { ghn3_set_error("msa lean: hidden %d not a multiple of 4 or above 1024", s.hidden); return GHN3_E_LIMIT; }
    const int64_t R = s.B * N;
    if (s.B > 65535 || R * 3 * s.C >= (1ll << 31) || R * s.hidden >= (1ll << 31)) {
        ghn3_set_error("msa lean: more than 65535 sequences, or activations of 2^31 elements or more");
        return GHN3_E_LIMIT;
    }
    if (out) {
        *out = MsaDims{s.B, s.H, s.W, s.C, s.heads, s.hidden, s.stride, s.Ho, s.Wo, s.layout, s.eps, (int)N, (int)R,
                       s.B * s.Ho * s.Wo};
    }
    return GHN3_OK;
}

// forward scratch: the saved-P layout, then lse [B][heads][N] (the last section: not rounded up, so that the lean state is never
// larger than the saved-P path's scratch and P together, a single token included)
int64_t lean_lse_off(const MsaDims& d) { return fwd_layout(d).total; }
int64_t lean_fwd_total(const MsaDims& d) { return lean_lse_off(d) + (int64_t)d.B * d.heads * d.N; }

template <int RB>
int lean_fwd_rb(const MsaDims& d, const float* x, const ghn3_msa_params& p, float* out, float* scratch, bool save, hipStream_t s) {
    const FwdLayout f = fwd_layout(d);
    int rc;
    if ((rc = tnet_raise_lds(msa_ln_qkv_kernel<RB>, MAX_LDS))) return rc;
    hipLaunchKernelGGL(msa_ln_qkv_kernel<RB>, dim3((d.R + RB - 1) / RB), dim3(NT), (size_t)RB * (r16(d.C) + 4) * 4, s, d, x, p,
                       scratch + f.qkv, scratch + f.stats1, reinterpret_cast<int*>(scratch + f.nn));
    TNET_LAUNCH_CHECK("msa lean ln_qkv");
    if ((rc = ghn3_attn_lean_fwd(scratch + f.O, save ? scratch + lean_lse_off(d) : nullptr, scratch + f.qkv, d.B, d.N, d.C,
                                 d.heads, s)))
        return rc;
    if ((rc = tnet_raise_lds(msa_post_kernel<RB>, MAX_LDS))) return rc;
    hipLaunchKernelGGL(msa_post_kernel<RB>, dim3((d.Kr + RB - 1) / RB), dim3(NT), (size_t)lds_post(RB, d), s, d, x,
                       (const float*)(scratch + f.O), p, out, save ? scratch + f.y1 : nullptr,
                       save ? scratch + f.stats2 : nullptr, save ? scratch + f.pre : nullptr);
    TNET_LAUNCH_CHECK("msa lean post");
    return GHN3_OK;
}

template <int RB>
int lean_bwd_rb(const MsaDims& d, const float* dout, const float* x, const ghn3_msa_params& p, const float* fs, float* dx,
                const ghn3_msa_grads& g, float* scratch, hipStream_t s) {
    const FwdLayout f = fwd_layout(d);
    const BwdLayout b = bwd_layout(d);
    int rc;
    if (d.Kr != d.R) {                           // (dropped rows: no gradient reaches them through y)
        hipError_t e = hipMemsetAsync(scratch + b.dO, 0, (size_t)(b.dy1 - b.dO + (int64_t)d.R * d.C) * sizeof(float), s);  // dO, dy1
        if (e != hipSuccess) { ghn3_set_error("msa lean bwd: hipMemsetAsync: %s", hipGetErrorString(e)); return GHN3_E_HIP; }
    }
    const int nb_post = (d.Kr + RB - 1) / RB, nb_rows = (d.R + RB - 1) / RB;
    if ((rc = tnet_raise_lds(msa_post_bwd_kernel<RB>, MAX_LDS))) return rc;
    hipLaunchKernelGGL(msa_post_bwd_kernel<RB>, dim3(nb_post), dim3(NT), (size_t)lds_post_bwd(RB, d), s, d, dout, p,
                       fs + f.y1, fs + f.stats2, fs + f.pre, scratch + b.dh, scratch + b.gact, scratch + b.a2, scratch + b.dy1,
                       scratch + b.dO, scratch + b.ln2);
    TNET_LAUNCH_CHECK("msa lean post bwd");
    if ((rc = ghn3_attn_lean_bwd(scratch + b.dqkv, scratch + b.dO, fs + f.qkv, fs + lean_lse_off(d), fs + f.O, d.B, d.N, d.C,
                                 d.heads, s)))
        return rc;
    if ((rc = tnet_raise_lds(msa_qkv_bwd_kernel<RB>, MAX_LDS))) return rc;
    hipLaunchKernelGGL(msa_qkv_bwd_kernel<RB>, dim3(nb_rows), dim3(NT), (size_t)lds_qkv_bwd(RB, d), s, d, x, p,
                       (const float*)(scratch + b.dqkv), fs + f.stats1, (const float*)(scratch + b.dy1), scratch + b.a1, dx,
                       scratch + b.ln1);
    TNET_LAUNCH_CHECK("msa lean qkv bwd");
    const TnetWgProb wg[4] = {
        {scratch + b.dqkv, scratch + b.a1, scratch + b.pq, g.w_qkv, g.b_qkv, d.R, 3 * d.C, d.C, g.b_qkv != nullptr},
        {scratch + b.dy1, fs + f.O, scratch + b.po, g.w_o, g.b_o, d.R, d.C, d.C, 1},
        {scratch + b.dh, scratch + b.a2, scratch + b.p1, g.w1, g.b1, d.Kr, d.hidden, d.C, 1},
        {dout, scratch + b.gact, scratch + b.p2, g.w2, g.b2, d.Kr, d.C, d.hidden, 1},
    };
    if ((rc = tnet_wgrad_launch(wg, 4, s))) return rc;
    const TnetRedProb red[6] = {
        tnet_wg_reduce(wg[0]), tnet_wg_reduce(wg[1]), tnet_wg_reduce(wg[2]), tnet_wg_reduce(wg[3]),
        {scratch + b.ln1, g.ln1_w, g.ln1_b, nb_rows, 2 * d.C, d.C, d.C, 1},
        {scratch + b.ln2, g.ln2_w, g.ln2_b, nb_post, 2 * d.C, d.C, d.C, 1},
    };
    return tnet_reduce_launch(red, 6, s);
}

}  // namespace

extern "C" int64_t ghn3_msa_lean_scratch_floats(const ghn3_msa_desc* desc, int backward) {
    MsaDims d;
    const int rc = check_lean(desc, &d);
    if (rc) return rc;
    return backward ? bwd_layout(d).total : lean_fwd_total(d);
}

extern "C" int ghn3_msa_lean_fwd(const ghn3_msa_desc* desc, const float* x, const ghn3_msa_params* params, float* out,
                                 float* scratch, int save, void* stream) {
    MsaDims d;
    int rc = check_lean(desc, &d);
    if (rc) return rc;
    if (!x || !out || !scratch || !params_ok(params, desc->has_qkv_bias) || !a16(x) || !a16(scratch)) {
        ghn3_set_error("msa lean fwd: null or misaligned pointer (x, scratch and the weight matrices need 16-byte alignment)");
        return GHN3_E_ARG;
    }
    ghn3_msa_params p = *params;
    if (!desc->has_qkv_bias) p.b_qkv = nullptr;
    hipStream_t s = (hipStream_t)stream;
    return pick_rb(d) == 32 ? lean_fwd_rb<32>(d, x, p, out, scratch, save != 0, s)
                            : lean_fwd_rb<16>(d, x, p, out, scratch, save != 0, s);
}

extern "C" int ghn3_msa_lean_bwd(const ghn3_msa_desc* desc, const float* dout, const float* x, const ghn3_msa_params* params,
                                 const float* fwd_scratch, float* dx, const ghn3_msa_grads* grads, float* scratch, void* stream) {
    MsaDims d;
    int rc = check_lean(desc, &d);
    if (rc) return rc;
    if (!dout || !x || !fwd_scratch || !dx || !scratch || !grads || !params_ok(params, desc->has_qkv_bias) || !a16(dout) ||
        !a16(x) || !a16(fwd_scratch) || !a16(dx) || !a16(scratch)) {
        ghn3_set_error("msa lean bwd: null or misaligned pointer");
        return GHN3_E_ARG;
    }
    const ghn3_msa_grads& g = *grads;
    if (!g.ln1_w || !g.ln1_b || !g.w_qkv || (desc->has_qkv_bias && !g.b_qkv) || !g.w_o || !g.b_o || !g.ln2_w || !g.ln2_b ||
        !g.w1 || !g.b1 || !g.w2 || !g.b2) {
        ghn3_set_error("msa lean bwd: null gradient pointer");
        return GHN3_E_ARG;
    }
    ghn3_msa_params p = *params;
    ghn3_msa_grads gg = g;
    if (!desc->has_qkv_bias) { p.b_qkv = nullptr; gg.b_qkv = nullptr; }
    hipStream_t s = (hipStream_t)stream;
    return pick_rb(d) == 32 ? lean_bwd_rb<32>(d, dout, x, p, fwd_scratch, dx, gg, scratch, s)
                            : lean_bwd_rb<16>(d, dout, x, p, fwd_scratch, dx, gg, scratch, s);
}
