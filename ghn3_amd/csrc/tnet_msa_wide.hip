// Target-network layers: the `msa` op for WIDE layers -- C <= 1024, head dim <= 64, hidden <= 4096 -- which the row-block kernels
// of tnet_msa.hip cannot hold in LDS (they keep a block's [RB][C] and [RB][hidden] images there and stream each weight matrix
// once per 16 - 32 token rows).  The layer is the one of tnet_msa.hip:
//
//     t  = tokens(x)                                                  (B, N = H W, C), x NCHW or NHWC
//     y1 = t + Wo attn(LN1(t) Wqkv^T [+ bqkv]) + bo
//     y  = y1 + W2 gelu_erf(W1 LN2(y1) + b1) + b2
//     out = y[::s, ::s]                                               NHWC (B, Ho, Wo, C)
//
// built from a few general kernels instead of fused row blocks:
//
//   wide_gemm      C [M][Nn] = sum_k A(m, k) B(n, k) on 64 x 64 output tiles, the reduction walked in 32-wide chunks through LDS
//                  (18 KB), either operand with its reduction index or its tile index contiguous in memory: one kernel for the
//                  linears (Y = A W^T), their data gradients (dA = G W) and their weight gradients (dW = G^T X, the token rows
//                  split into a shape-fixed number of chunks whose partial products tnet_reduce sums in chunk order).  A weight
//                  matrix is read once per 64 token rows.  Epilogues: bias (+ residual); bias, pre-GELU value and GELU; times
//                  GELU' of the saved pre-GELU value.  v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulate.
//   wide_ln_fwd    LayerNorm of token rows, a wave per row (the row stays in registers); writes the normalised rows and
//                  (mean, rstd);
//   wide_ln_bwd    LayerNorm backward of 64 rows per workgroup (+ the residual gradient), and the workgroup's partial sums of the
//                  LayerNorm parameter gradients, rows in order;
//   wide_transpose NCHW <-> NHWC (only for an NCHW x), wide_rows_copy the kept rows behind `stride` (only for stride > 1),
//   wide_colsum    the bias gradients as fixed row-chunk partial column sums;
//   attn_wide      the lean attention of tnet_attn.hip (no saved P: lse per query row, P recomputed in the backward) for
//                  32 < d <= 64: a score tile takes up to 32 k-steps of v_mfma_f32_32x32x2_f32, and the O, dQ, dK and dV
//                  products span two 32-column halves of the head, each with an accumulator tile of its own.  d <= 32 launches
//                  the kernels of tnet_attn.hip through ghn3_attn_lean_*.
//
// No float atomics anywhere; every partial sum is reduced in a fixed order: reruns are bit-identical.  An inference forward and a
// training forward launch the same kernels with the same arguments.

#include <math.h>
#include <algorithm>
#include "tnet_common.h"

namespace {

constexpr int NT = 256;                     // threads per workgroup (4 waves)

struct WideDims {
    int B, H, W, C, heads, hidden, stride, Ho, Wo, layout;
    float eps;
    int N, R, Kr;                           // tokens per sequence, token rows B N, kept rows B Ho Wo
};

__device__ inline float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
__device__ inline float gelu_erf_grad(float v) {
    return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * expf(-0.5f * v * v);
}

// ------------------------------------------------------------------------------------------------ the product kernel
constexpr int GT = 64;                      // output tile (rows and columns)
constexpr int GK = 32;                      // reduction chunk
constexpr int GLD = GK + 4;                 // LDS row pitch in floats (144 bytes: float4-aligned rows)

enum { EPI_BIAS_RES = 0, EPI_GELU = 1, EPI_DGELU = 2 };

// C [z][m][n] = sum over k in chunk z of A(m, k) B(n, k).  XM = false: element (m, k) of the operand at X[m ld + k] (the
// reduction index contiguous; K % 4 == 0); XM = true: at X[k ld + m] (the tile index contiguous; its extent % 4 == 0).
struct WGemm {
    const float* A; const float* B; float* C;
    int M, Nn, K, lda, ldb, ldc;
    int kper;                               // reduction elements per chunk (a multiple of GK); gridDim.z chunks
    size_t cstride;                         // floats between the outputs of two chunks
    const float* bias;                      // [Nn] or null                                   (EPI_BIAS_RES, EPI_GELU)
    const float* res;                       // [M][ldc] added to the output, or null          (EPI_BIAS_RES)
    const float* aux;                       // [M][ldc] pre-GELU values                       (EPI_DGELU)
    float* out2;                            // [M][ldc] gelu(output)                          (EPI_GELU)
};

// the two float4 a thread holds of a 64 x 32 operand tile (zero outside the operand)
template <bool XM>
__device__ __forceinline__ void tile_fetch(const float* __restrict__ X, int ld, int t0, int T, int k0, int ke, int tid, f32x4 (&r)[2]) {
    const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!XM) {
        const int t = t0 + (tid >> 2), k = k0 + (tid & 3) * 8;
        const float* p = X + (size_t)t * ld + k;
        r[0] = (t < T && k < ke) ? *reinterpret_cast<const f32x4*>(p) : z;
        r[1] = (t < T && k + 4 < ke) ? *reinterpret_cast<const f32x4*>(p + 4) : z;
    } else {
        const int t = t0 + (tid & 15) * 4, k = k0 + (tid >> 4);
        const float* p = X + (size_t)k * ld + t;
        r[0] = (t < T && k < ke) ? *reinterpret_cast<const f32x4*>(p) : z;
        r[1] = (t < T && k + 16 < ke) ? *reinterpret_cast<const f32x4*>(p + (size_t)16 * ld) : z;
    }
}
template <bool XM>
__device__ __forceinline__ void tile_put(float* S, int tid, const f32x4 (&r)[2]) {
    if (!XM) {
        float* p = S + (tid >> 2) * GLD + (tid & 3) * 8;
        *reinterpret_cast<f32x4*>(p) = r[0];
        *reinterpret_cast<f32x4*>(p + 4) = r[1];
    } else {
        float* p = S + (tid & 15) * 4 * GLD + (tid >> 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { p[j * GLD] = r[0][j]; p[j * GLD + 16] = r[1][j]; }
    }
}

template <bool AM, bool BM, int EPI>
__global__ __launch_bounds__(NT) void wide_gemm_kernel(WGemm g) {
    __shared__ float As[GT * GLD], Bs[GT * GLD];
    const int m0 = blockIdx.x * GT, n0 = blockIdx.y * GT;
    const int kb = blockIdx.z * g.kper, ke = min(g.K, kb + g.kper);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ra[2], rb[2];
    tile_fetch<AM>(g.A, g.lda, m0, g.M, kb, ke, tid, ra);
    tile_fetch<BM>(g.B, g.ldb, n0, g.Nn, kb, ke, tid, rb);
    for (int k0 = kb; k0 < ke; k0 += GK) {
        tile_put<AM>(As, tid, ra);
        tile_put<BM>(Bs, tid, rb);
        __syncthreads();
        if (k0 + GK < ke) {                                           // (the next chunk's loads fly behind this chunk's products)
            tile_fetch<AM>(g.A, g.lda, m0, g.M, k0 + GK, ke, tid, ra);
            tile_fetch<BM>(g.B, g.ldb, n0, g.Nn, k0 + GK, ke, tid, rb);
        }
#pragma unroll
        for (int h = 0; h < GK / 16; ++h) {
            f32x4 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *reinterpret_cast<const f32x4*>(As + (wm + t * 16 + i) * GLD + 16 * h + 4 * q);
                b[t] = *reinterpret_cast<const f32x4*>(Bs + (wn + t * 16 + i) * GLD + 16 * h + 4 * q);
            }
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][j], b[ct][j], acc[rt][ct], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D: row 4 (lane >> 4) + reg, col lane & 15
    float* C = g.C + blockIdx.z * g.cstride;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + rt * 16 + 4 * q + r, n = n0 + wn + ct * 16 + i;
                if (m >= g.M || n >= g.Nn) continue;
                const size_t e = (size_t)m * g.ldc + n;
                float v = acc[rt][ct][r];
                if (EPI == EPI_BIAS_RES) {
                    if (g.bias) v += g.bias[n];
                    if (g.res) v += g.res[e];
                    C[e] = v;
                } else if (EPI == EPI_GELU) {
                    v += g.bias[n];
                    C[e] = v;
                    g.out2[e] = gelu_erf(v);
                } else {
                    C[e] = v * gelu_erf_grad(g.aux[e]);
                }
            }
}

template <bool AM, bool BM, int EPI>
int gemm_launch(const char* what, const WGemm& g, int chunks, hipStream_t s) {
    hipLaunchKernelGGL((wide_gemm_kernel<AM, BM, EPI>), dim3((g.M + GT - 1) / GT, (g.Nn + GT - 1) / GT, chunks), dim3(NT), 0, s, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ghn3_set_error("msa wide %s: %s", what, hipGetErrorString(e)); return GHN3_E_HIP; }
    return GHN3_OK;
}

// Y [M][Nn] = A [M][K] W^T (W [Nn][K]) + bias (+ res)
int linear_fwd(const char* what, const float* A, const float* W, const float* bias, const float* res, float* Y, int M, int Nn, int K,
               hipStream_t s) {
    const WGemm g{A, W, Y, M, Nn, K, K, K, Nn, (K + GK - 1) / GK * GK, 0, bias, res, nullptr, nullptr};
    return gemm_launch<false, false, EPI_BIAS_RES>(what, g, 1, s);
}
// dA [M][K] = G [M][Nn] W (W [Nn][K]); aux != null: times gelu'(aux)
int linear_dgrad(const char* what, const float* G, const float* W, const float* aux, float* dA, int M, int Nn, int K, hipStream_t s) {
    const WGemm g{G, W, dA, M, K, Nn, Nn, K, K, (Nn + GK - 1) / GK * GK, 0, nullptr, nullptr, aux, nullptr};
    return aux ? gemm_launch<false, true, EPI_DGELU>(what, g, 1, s) : gemm_launch<false, true, EPI_BIAS_RES>(what, g, 1, s);
}

// The weight gradient dW [Nout][K] = G^T X over `rows` rows: the rows are split into wg_chunks(...) chunks -- a function of the
// shape alone -- so that a narrow weight still fills the device; one chunk writes dW itself.
struct WgPlan { int chunks, per; };
WgPlan wg_plan(int rows, int Nout, int K) {
    const int64_t tiles = (int64_t)((Nout + GT - 1) / GT) * ((K + GT - 1) / GT);
    int want = (int)std::max<int64_t>(1, 512 / tiles);
    want = std::min(std::min(want, 16), (rows + 127) / 128);
    const int per = ((rows + want - 1) / want + GK - 1) / GK * GK;
    return WgPlan{(rows + per - 1) / per, per};
}
int64_t wg_part_floats(int rows, int Nout, int K) {
    const WgPlan p = wg_plan(rows, Nout, K);
    return p.chunks > 1 ? al((int64_t)p.chunks * Nout * K) : 0;
}
int linear_wgrad(const char* what, const float* G, const float* X, float* part, float* dW, int rows, int Nout, int K, hipStream_t s,
                 TnetRedProb* red, int* n_red) {
    const WgPlan p = wg_plan(rows, Nout, K);
    const bool split = p.chunks > 1;
    const WGemm g{G, X, split ? part : dW, Nout, K, rows, Nout, K, K, p.per, (size_t)Nout * K, nullptr, nullptr, nullptr, nullptr};
    if (split) red[(*n_red)++] = TnetRedProb{part, dW, nullptr, p.chunks, Nout * K, K, K, 0};
    return gemm_launch<true, true, EPI_BIAS_RES>(what, g, p.chunks, s);
}

// ------------------------------------------------------------------------------------------------ row kernels
// LayerNorm of `rows` rows of C <= 1024 floats, a wave per row: two-pass biased variance as torch
__global__ __launch_bounds__(NT) void wide_ln_fwd_kernel(const float* __restrict__ x, int rows, int C, float eps,
                                                         const float* __restrict__ gam, const float* __restrict__ bet,
                                                         float* __restrict__ a, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * (NT / 64) + wave;
    if (r >= rows) return;
    const float* xr = x + (size_t)r * C;
    f32x4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * lane + 256 * i;
        v[i] = c < C ? *reinterpret_cast<const f32x4*>(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (4 * lane + 256 * i < C) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float t = v[i][j] - mean; q += t * t; }
        }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * lane + 256 * i;
        if (c < C) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (v[i][j] - mean) * rstd * gam[c + j] + bet[c + j];
            *reinterpret_cast<f32x4*>(a + (size_t)r * C + c) = o;
        }
    }
    if (lane == 0) { stats[2 * (size_t)r] = mean; stats[2 * (size_t)r + 1] = rstd; }
}

// LayerNorm backward of LNB rows per workgroup: dx = res + rstd (dxh - mean(dxh) - xhat mean(dxh xhat)), dxh = da . gamma, and
// the workgroup's partial sums part [block][2 C] = (sum da . xhat | sum da), rows in order
constexpr int LNB = 64;
__global__ __launch_bounds__(NT) void wide_ln_bwd_kernel(const float* __restrict__ da, const float* __restrict__ x,
                                                         const float* __restrict__ stats, const float* __restrict__ gam,
                                                         const float* __restrict__ res, float* __restrict__ dx,
                                                         float* __restrict__ part, int rows, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * LNB, r1 = min(rows, r0 + LNB);
    for (int r = r0 + wave; r < r1; r += NT / 64) {
        const float mean = stats[2 * (size_t)r], rstd = stats[2 * (size_t)r + 1];
        const size_t o = (size_t)r * C;
        f32x4 xh[4], dxh[4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 4 * lane + 256 * i;
            if (c < C) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(x + o + c), dv = *reinterpret_cast<const f32x4*>(da + o + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    xh[i][j] = (xv[j] - mean) * rstd;
                    dxh[i][j] = dv[j] * gam[c + j];
                    s1 += dxh[i][j];
                    s2 += dxh[i][j] * xh[i][j];
                }
            }
        }
        s1 = wave_sum(s1) / (float)C;
        s2 = wave_sum(s2) / (float)C;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 4 * lane + 256 * i;
            if (c < C) {
                f32x4 g = res ? *reinterpret_cast<const f32x4*>(res + o + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] += rstd * (dxh[i][j] - s1 - xh[i][j] * s2);
                *reinterpret_cast<f32x4*>(dx + o + c) = g;
            }
        }
    }
    for (int c = threadIdx.x; c < C; c += NT) {
        float sg = 0.f, sb = 0.f;
        for (int r = r0; r < r1; ++r) {
            const float mean = stats[2 * (size_t)r], rstd = stats[2 * (size_t)r + 1];
            const float dv = da[(size_t)r * C + c];
            sg += dv * ((x[(size_t)r * C + c] - mean) * rstd);
            sb += dv;
        }
        part[(size_t)blockIdx.x * 2 * C + c] = sg;
        part[(size_t)blockIdx.x * 2 * C + C + c] = sb;
    }
}

// dst [z][cols][rows] = src [z][rows][cols]^T, 32 x 32 tiles through LDS
__global__ __launch_bounds__(NT) void wide_transpose_kernel(float* __restrict__ dst, const float* __restrict__ src, int rows, int cols) {
    __shared__ float tile[32][33];
    const size_t base = (size_t)blockIdx.z * rows * cols;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < rows && c0 + tx < cols) tile[j][tx] = src[base + (size_t)(r0 + j) * cols + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < cols && r0 + tx < rows) dst[base + (size_t)(c0 + j) * rows + r0 + tx] = tile[tx][j];
}

// kept row kr <-> token row; scatter == 0: dst[kr] = src[token row], else dst[token row] = src[kr]
__global__ __launch_bounds__(NT) void wide_rows_copy_kernel(float* __restrict__ dst, const float* __restrict__ src, WideDims d, int scatter) {
    const int kr = blockIdx.x;
    const int hw = d.Ho * d.Wo, b = kr / hw, p = kr - b * hw, ho = p / d.Wo, wo = p - ho * d.Wo;
    const size_t tr = (size_t)b * d.N + (size_t)ho * d.stride * d.W + wo * d.stride;
    const float* s = src + (scatter ? (size_t)kr : tr) * d.C;
    float* t = dst + (scatter ? tr : (size_t)kr) * d.C;
    for (int c = 4 * threadIdx.x; c < d.C; c += 4 * NT) *reinterpret_cast<f32x4*>(t + c) = *reinterpret_cast<const f32x4*>(s + c);
}

// part [chunk][Nout] = column sums of rows [chunk rper, (chunk + 1) rper) of G [rows][Nout], rows in order
__global__ __launch_bounds__(NT) void wide_colsum_kernel(const float* __restrict__ G, int rows, int Nout, int rper, float* __restrict__ part) {
    const int n = blockIdx.x * NT + threadIdx.x;
    if (n >= Nout) return;
    const int rb = blockIdx.y * rper, re = min(rows, rb + rper);
    float s = 0.f;
    for (int r = rb; r < re; ++r) s += G[(size_t)r * Nout + n];
    part[(size_t)blockIdx.y * Nout + n] = s;
}
struct CsPlan { int chunks, per; };
CsPlan cs_plan(int rows) {
    const int want = std::min((rows + 63) / 64, 512);
    const int per = (rows + want - 1) / want;
    return CsPlan{(rows + per - 1) / per, per};
}
int64_t cs_part_floats(int rows, int Nout) { return al((int64_t)cs_plan(rows).chunks * Nout); }

// ------------------------------------------------------------------------------------------------ attention, 32 < d <= 64
// The operand helpers and the tile orientation are those of tnet_attn.hip (whose kernels stay as they are): a score-shaped
// 32 x 32 tile has the owned index on the lane and the streamed index in the 16 accumulator registers.  Here the head columns
// e = 32 hh + (lane & 31), hh = 0, 1, are two halves with an accumulator tile each.
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int AW = 4;                       // waves per workgroup
constexpr int WIDE_DMAX = 64, WIDE_NMAX = 4096;

__device__ __forceinline__ int acc_row(int r, int lhi) { return (r & 3) + 8 * (r >> 2) + 4 * lhi; }
__device__ __forceinline__ f32x16 splat16(float v) {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = v;
    return z;
}
// x[s] = mul X[row][2 s + lhi], zero for k >= d or row >= n_rows; loads unconditional (clamped), values selected afterwards
template <int KS>
__device__ __forceinline__ void row_operand(const float* __restrict__ X, int row, int n_rows, size_t stride, int d, int lhi,
                                            bool vec, float mul, float (&x)[KS]) {
    const bool ok = row < n_rows;
    const float* r = X + (size_t)min(row, n_rows - 1) * stride;
    if (vec) {
        f32x4 f[KS / 2];
#pragma unroll
        for (int c = 0; c < KS / 2; ++c) f[c] = *reinterpret_cast<const f32x4*>(r + min(4 * c, d - 4));
#pragma unroll
        for (int c = 0; c < KS / 2; ++c) {
            const bool on = ok && 4 * c < d;
            x[2 * c] = on ? mul * (lhi ? f[c].y : f[c].x) : 0.f;
            x[2 * c + 1] = on ? mul * (lhi ? f[c].w : f[c].z) : 0.f;
        }
    } else {
        float v[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) v[s] = r[min(2 * s + lhi, d - 1)];
#pragma unroll
        for (int s = 0; s < KS; ++s) x[s] = (ok && 2 * s + lhi < d) ? mul * v[s] : 0.f;
    }
}
// x[s] = X[row0 + acc_row(s, lhi)][e], zero for e >= d or rows >= n_rows
__device__ __forceinline__ void col_operand(const float* __restrict__ X, int row0, int n_rows, size_t stride, int e, int d,
                                            int lhi, float (&x)[16]) {
    const int ec = min(e, d - 1);
    float v[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) v[s] = X[(size_t)min(row0 + acc_row(s, lhi), n_rows - 1) * stride + ec];
#pragma unroll
    for (int s = 0; s < 16; ++s) x[s] = (e < d && row0 + acc_row(s, lhi) < n_rows) ? v[s] : 0.f;
}
template <int KS>
__device__ __forceinline__ f32x16 mfma_rows(const float (&a)[KS], const float (&b)[KS], f32x16 acc) {
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ f32x16 mfma_cols(const float (&a)[16], const f32x16& b, f32x16 acc) {
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    return acc;
}
// sum of the waves' partial tiles through LDS in wave order; wave w returns the head columns 8 w + 4 lhi + c of its half
__device__ __forceinline__ f32x4 reduce_waves(float* red /* [AW][16][64] */, const f32x16& part, int w, int lane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(w * 16 + r) * 64 + lane] = part[r];
    __syncthreads();
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int r = 4 * w + c;
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < AW; ++q) t += red[(16 * q + r) * 64 + lane];
        o[c] = t;
    }
    __syncthreads();                                                  // (the buffer is free for the next half)
    return o;
}
__device__ __forceinline__ void store4(float* __restrict__ dst, int e0, int d, bool vec, f32x4 v) {
    if (vec && e0 + 3 < d) {
        *reinterpret_cast<f32x4*>(dst + e0) = v;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (e0 + c < d) dst[e0 + c] = v[c];
    }
}
template <int KS>
__device__ __forceinline__ f32x16 score_tile(const float* __restrict__ Kb, const float (&qb)[KS], int j0, int N, int C, int d,
                                             int l31, int lhi, bool vec) {
    float ka[KS];
    row_operand<KS>(Kb, j0 + l31, N, (size_t)3 * C, d, lhi, vec, 1.f, ka);
    f32x16 acc = mfma_rows<KS>(ka, qb, splat16(0.f));
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (j0 + acc_row(r, lhi) >= N) acc[r] = -INFINITY;
    return acc;
}

// forward: grid (ceil(N / 32), heads, B); two passes over the key tiles as attn_lean_fwd_kernel
template <int KS>
__global__ __launch_bounds__(64 * AW, 2) void attn_wide_fwd_kernel(float* __restrict__ out, float* __restrict__ lse,
                                                                   const float* __restrict__ qkv, int N, int C, int H, float scale,
                                                                   int vec16) {
    __shared__ float red[AW * 16 * 64];
    __shared__ float red_m[AW][32], red_l[AW][32];
    const int d = C / H;
    const int NB = (N + 31) >> 5;
    const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * 32;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
    const float* base = qkv + (size_t)b * N * 3 * C + h * d;
    const size_t bh = ((size_t)b * H + h) * N;
    const int qi = i0 + l31;
    const bool vec = (d & 3) == 0 && vec16;
    float qb[KS];
    row_operand<KS>(base, qi, N, (size_t)3 * C, d, lhi, vec, scale, qb);

    float mx = -INFINITY, sum = 0.f;
    for (int t = w; t < NB; t += AW) {
        const f32x16 sc = score_tile<KS>(base + C, qb, t * 32, N, C, d, l31, lhi, vec);
        float tm = mx;
#pragma unroll
        for (int r = 0; r < 16; ++r) tm = fmaxf(tm, sc[r]);
        float acc = sum * expf(mx - tm);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc += expf(sc[r] - tm);
        sum = acc;
        mx = tm;
    }
    {
        const float m2 = __shfl_xor(mx, 32, 64), s2 = __shfl_xor(sum, 32, 64);
        const float mn = fmaxf(mx, m2);
        sum = (mx > -INFINITY ? sum * expf(mx - mn) : 0.f) + (m2 > -INFINITY ? s2 * expf(m2 - mn) : 0.f);
        mx = mn;
    }
    if (lhi == 0) { red_m[w][l31] = mx; red_l[w][l31] = sum; }
    __syncthreads();
    float gm = red_m[0][l31];
#pragma unroll
    for (int k = 1; k < AW; ++k) gm = fmaxf(gm, red_m[k][l31]);
    float gl = 0.f;
#pragma unroll
    for (int k = 0; k < AW; ++k)
        if (red_m[k][l31] > -INFINITY) gl += red_l[k][l31] * expf(red_m[k][l31] - gm);
    const float inv = 1.f / gl;
    if (lse && w == 0 && lhi == 0 && qi < N) lse[bh + qi] = gm + logf(gl);

    f32x16 O0 = splat16(0.f), O1 = splat16(0.f);
    for (int t = w; t < NB; t += AW) {
        const int j0 = t * 32;
        f32x16 sc = score_tile<KS>(base + C, qb, j0, N, C, d, l31, lhi, vec);
        float va0[16], va1[16];
        col_operand(base + 2 * C, j0, N, (size_t)3 * C, l31, d, lhi, va0);
        col_operand(base + 2 * C, j0, N, (size_t)3 * C, 32 + l31, d, lhi, va1);
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = expf(sc[r] - gm) * inv;
        O0 = mfma_cols(va0, sc, O0);
        O1 = mfma_cols(va1, sc, O1);
    }
    const f32x4 o0 = reduce_waves(red, O0, w, lane);
    const f32x4 o1 = reduce_waves(red, O1, w, lane);
    if (qi < N) {
        float* row = out + ((size_t)b * N + qi) * C + h * d;
        store4(row, 8 * w + 4 * lhi, d, vec, o0);
        store4(row, 32 + 8 * w + 4 * lhi, d, vec, o1);
    }
}

// backward: grid (2 ceil(N / 32), heads, B), the row and column roles of attn_lean_bwd_kernel.  One workgroup per CU
// (__launch_bounds__(256, 1)): a wave has the SIMD's whole unified register file, 512 registers.
template <int KS>
__global__ __launch_bounds__(64 * AW, 1) void attn_wide_bwd_kernel(float* __restrict__ dqkv, const float* __restrict__ dO,
                                                                   const float* __restrict__ qkv, const float* __restrict__ lse,
                                                                   const float* __restrict__ Oin, int N, int C, int H, float scale,
                                                                   int vec16) {
    __shared__ float red[AW * 16 * 64];
    __shared__ float dl[AW][32], ll[AW][32];
    const int d = C / H;
    const int NB = (N + 31) >> 5;
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
    const float* base = qkv + (size_t)b * N * 3 * C + h * d;
    const float* dOb = dO + (size_t)b * N * C + h * d;
    const float* Ob = Oin + (size_t)b * N * C + h * d;
    const float* lb = lse + ((size_t)b * H + h) * N;
    const size_t s3 = (size_t)3 * C, s1 = (size_t)C;
    const bool vec = (d & 3) == 0 && vec16;

    if ((int)blockIdx.x < NB) {
        // ---------------- row role: lane = query qi, accumulator registers = keys ----------------
        const int qi = blockIdx.x * 32 + l31;
        const bool qok = qi < N;
        float qb[KS], gb[KS];
        row_operand<KS>(base, qi, N, s3, d, lhi, vec, scale, qb);
        row_operand<KS>(dOb, qi, N, s1, d, lhi, vec, 1.f, gb);
        float delta = 0.f;
        {
            float ob[KS];
            row_operand<KS>(Ob, qi, N, s1, d, lhi, vec, 1.f, ob);
#pragma unroll
            for (int s = 0; s < KS; ++s) delta += gb[s] * ob[s];
        }
        delta += __shfl_xor(delta, 32, 64);
        const float lq = lb[min(qi, N - 1)];
        const f32x16 s_init = splat16(qok ? -lq : 0.f), dp_init = splat16(-delta);
        f32x16 dQ0 = splat16(0.f), dQ1 = splat16(0.f);
        for (int t = w; t < NB; t += AW) {
            const int j0 = t * 32;
            f32x16 sc, ds;
            {
                float ka[KS];
                row_operand<KS>(base + C, j0 + l31, N, s3, d, lhi, vec, 1.f, ka);
                sc = mfma_rows<KS>(ka, qb, s_init);                    // scale K Q^T - lse
            }
            {
                float va[KS];
                row_operand<KS>(base + 2 * C, j0 + l31, N, s3, d, lhi, vec, 1.f, va);
                ds = mfma_rows<KS>(va, gb, dp_init);                   // V dO^T - delta
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = (qok && j0 + acc_row(r, lhi) < N) ? expf(sc[r]) : 0.f;
                ds[r] = p * ds[r];
            }
            float kc[16];
            col_operand(base + C, j0, N, s3, l31, d, lhi, kc);
            dQ0 = mfma_cols(kc, ds, dQ0);                              // dQ^T += K^T dS^T, columns 0 .. 31
            col_operand(base + C, j0, N, s3, 32 + l31, d, lhi, kc);
            dQ1 = mfma_cols(kc, ds, dQ1);                              //                  columns 32 .. 63
        }
        f32x4 o0 = reduce_waves(red, dQ0, w, lane);
        f32x4 o1 = reduce_waves(red, dQ1, w, lane);
#pragma unroll
        for (int c = 0; c < 4; ++c) { o0[c] *= scale; o1[c] *= scale; }
        if (qok) {
            float* row = dqkv + ((size_t)b * N + qi) * s3 + h * d;
            store4(row, 8 * w + 4 * lhi, d, vec, o0);
            store4(row, 32 + 8 * w + 4 * lhi, d, vec, o1);
        }
    } else {
        // ---------------- column role: lane = key kj, accumulator registers = queries ----------------
        const int kj = (blockIdx.x - NB) * 32 + l31;
        const bool kok = kj < N;
        float kb[KS], vb[KS];
        row_operand<KS>(base + C, kj, N, s3, d, lhi, vec, 1.f, kb);
        row_operand<KS>(base + 2 * C, kj, N, s3, d, lhi, vec, 1.f, vb);
        f32x16 dV0 = splat16(0.f), dV1 = splat16(0.f), dK0 = splat16(0.f), dK1 = splat16(0.f);
        for (int t = w; t < NB; t += AW) {
            const int q0 = t * 32, qrow = q0 + l31;
            float qa[KS], ga[KS];
            row_operand<KS>(base, qrow, N, s3, d, lhi, vec, scale, qa);
            row_operand<KS>(dOb, qrow, N, s1, d, lhi, vec, 1.f, ga);
            float dpart = 0.f;
            {
                float oa[KS];
                row_operand<KS>(Ob, qrow, N, s1, d, lhi, vec, 1.f, oa);
#pragma unroll
                for (int s = 0; s < KS; ++s) dpart += ga[s] * oa[s];
            }
            dpart += __shfl_xor(dpart, 32, 64);
            const float lq = lb[min(qrow, N - 1)];
            // wave-private hand-off of the row constants: lane (query) -> accumulator register index
            if (lhi == 0) { dl[w][l31] = -dpart; ll[w][l31] = qrow < N ? -lq : 0.f; }
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            f32x16 sc, ds;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sc[r] = ll[w][acc_row(r, lhi)]; ds[r] = dl[w][acc_row(r, lhi)]; }
            sc = mfma_rows<KS>(qa, kb, sc);                            // scale S - lse   (rows = queries, lane = key)
            ds = mfma_rows<KS>(ga, vb, ds);                            // dO V^T - delta
            f32x16 p;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = (kok && q0 + acc_row(r, lhi) < N) ? expf(sc[r]) : 0.f;
                ds[r] = p[r] * ds[r];
            }
            __builtin_amdgcn_wave_barrier();                           // (the next tile rewrites dl and ll)
            float xc[16];
            col_operand(dOb, q0, N, s1, l31, d, lhi, xc);
            dV0 = mfma_cols(xc, p, dV0);                               // dV^T += dO^T P
            col_operand(dOb, q0, N, s1, 32 + l31, d, lhi, xc);
            dV1 = mfma_cols(xc, p, dV1);
            col_operand(base, q0, N, s3, l31, d, lhi, xc);
            dK0 = mfma_cols(xc, ds, dK0);                              // dK^T += Q^T dS
            col_operand(base, q0, N, s3, 32 + l31, d, lhi, xc);
            dK1 = mfma_cols(xc, ds, dK1);
        }
        const f32x4 v0 = reduce_waves(red, dV0, w, lane);
        const f32x4 v1 = reduce_waves(red, dV1, w, lane);
        f32x4 k0 = reduce_waves(red, dK0, w, lane);
        f32x4 k1 = reduce_waves(red, dK1, w, lane);
#pragma unroll
        for (int c = 0; c < 4; ++c) { k0[c] *= scale; k1[c] *= scale; }
        if (kok) {
            float* row = dqkv + ((size_t)b * N + kj) * s3 + h * d;
            store4(row + 2 * C, 8 * w + 4 * lhi, d, vec, v0);
            store4(row + 2 * C, 32 + 8 * w + 4 * lhi, d, vec, v1);
            store4(row + C, 8 * w + 4 * lhi, d, vec, k0);
            store4(row + C, 32 + 8 * w + 4 * lhi, d, vec, k1);
        }
    }
}

int attn_check(const char* what, int B, int N, int C, int H) {
    if (B <= 0 || B > 65535 || H <= 0 || H > 65535 || C <= 0 || C % 4 || C % H || C / H > WIDE_DMAX) {
        ghn3_set_error("%s: needs 1 <= B, heads <= 65535, C %% 4 == 0, C %% heads == 0 and head dim <= %d (B %d, C %d, heads %d)",
                       what, WIDE_DMAX, B, C, H);
        return GHN3_E_LIMIT;
    }
    if (N <= 0 || N > WIDE_NMAX) { ghn3_set_error("%s: N = %d outside [1, %d]", what, N, WIDE_NMAX); return GHN3_E_LIMIT; }
    return GHN3_OK;
}
bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int ghn3_attn_wide_fwd(float* out, float* lse, const float* qkv, int B, int N, int C, int heads, void* stream) {
    int rc = attn_check("wide attention fwd", B, N, C, heads);
    if (rc) return rc;
    if (!out || !qkv) { ghn3_set_error("wide attention fwd: null pointer"); return GHN3_E_ARG; }
    const int d = C / heads, nb = (N + 31) / 32;
    if (d <= 32) return ghn3_attn_lean_fwd(out, lse, qkv, B, N, C, heads, stream);
    const float scale = 1.0f / sqrtf((float)d);
    const int vec = a16(out) && a16(qkv);
    auto fn = d <= 40 ? attn_wide_fwd_kernel<20> : d <= 48 ? attn_wide_fwd_kernel<24> : attn_wide_fwd_kernel<32>;
    hipLaunchKernelGGL(fn, dim3(nb, heads, B), dim3(64 * AW), 0, (hipStream_t)stream, out, lse, qkv, N, C, heads, scale, vec);
    TNET_LAUNCH_CHECK("wide attention fwd");
    return GHN3_OK;
}

extern "C" int ghn3_attn_wide_bwd(float* dqkv, const float* dO, const float* qkv, const float* lse, const float* O, int B, int N,
                                  int C, int heads, void* stream) {
    int rc = attn_check("wide attention bwd", B, N, C, heads);
    if (rc) return rc;
    if (!dqkv || !dO || !qkv || !lse || !O) {
        ghn3_set_error("wide attention bwd: null pointer (needs the forward's lse and output)");
        return GHN3_E_ARG;
    }
    const int d = C / heads, nb = (N + 31) / 32;
    if (d <= 32) return ghn3_attn_lean_bwd(dqkv, dO, qkv, lse, O, B, N, C, heads, stream);
    const float scale = 1.0f / sqrtf((float)d);
    const int vec = a16(dqkv) && a16(dO) && a16(qkv) && a16(O);
    auto fn = d <= 40 ? attn_wide_bwd_kernel<20> : d <= 48 ? attn_wide_bwd_kernel<24> : attn_wide_bwd_kernel<32>;
    hipLaunchKernelGGL(fn, dim3(2 * nb, heads, B), dim3(64 * AW), 0, (hipStream_t)stream, dqkv, dO, qkv, lse, O, N, C, heads, scale,
                       vec);
    TNET_LAUNCH_CHECK("wide attention bwd");
    return GHN3_OK;
}

// ------------------------------------------------------------------------------------------------ the layer, host side
namespace {

int check_wide(const ghn3_msa_desc* g, WideDims* out) {
    if (!g) { ghn3_set_error("msa wide: null descriptor"); return GHN3_E_ARG; }
    const ghn3_msa_desc& s = *g;
    if (s.B <= 0 || s.H <= 0 || s.W <= 0 || s.C <= 0 || s.heads <= 0 || s.hidden <= 0 || s.stride <= 0 || s.Ho <= 0 || s.Wo <= 0) {
        ghn3_set_error("msa wide: non-positive size in the descriptor");
        return GHN3_E_ARG;
    }
    if (s.layout != 0 && s.layout != 1) { ghn3_set_error("msa wide: layout %d is neither 0 (NCHW) nor 1 (NHWC)", s.layout); return GHN3_E_ARG; }
    if (s.Ho != (s.H - 1) / s.stride + 1 || s.Wo != (s.W - 1) / s.stride + 1) {
        ghn3_set_error("msa wide: output grid %d x %d does not match H, W, stride", s.Ho, s.Wo);
        return GHN3_E_ARG;
    }
    const int64_t N = (int64_t)s.H * s.W;
    if (s.C % 4 || s.C > 1024 || s.C % s.heads || s.C / s.heads > WIDE_DMAX) {
        ghn3_set_error("msa wide: needs C %% 4 == 0, C <= 1024, C %% heads == 0 and head dim <= %d (C %d, heads %d)", WIDE_DMAX, s.C,
                       s.heads);
        return GHN3_E_LIMIT;
    }
    if (N > WIDE_NMAX) { ghn3_set_error("msa wide: %lld tokens per sequence (limit %d)", (long long)N, WIDE_NMAX); return GHN3_E_LIMIT; }
    if (s.hidden % 4 || s.hidden > 4096) { ghn3_set_error("msa wide: hidden %d not a multiple of 4 or above 4096", s.hidden); return GHN3_E_LIMIT; }
    const int64_t R = s.B * N;
    if (s.B > 65535 || R * 3 * s.C >= (1ll << 31) || R * s.hidden >= (1ll << 31)) {
        ghn3_set_error("msa wide: more than 65535 sequences, or activations of 2^31 elements or more");
        return GHN3_E_LIMIT;
    }
    if (out) {
        *out = WideDims{s.B, s.H, s.W, s.C, s.heads, s.hidden, s.stride, s.Ho, s.Wo, s.layout, s.eps, (int)N, (int)R,
                        s.B * s.Ho * s.Wo};
    }
    return GHN3_OK;
}

// forward scratch: t (NCHW input only) | a1 | stats1 | qkv | O | Ok, tk (stride > 1 only: the kept rows of O and t) | y1 | a2 |
// stats2 | pre | gact | lse
struct FwdLayout { int64_t t, a1, stats1, qkv, O, Ok, tk, y1, a2, stats2, pre, gact, lse, total; };
FwdLayout fwd_layout(const WideDims& d) {
    FwdLayout f;
    const int64_t RC = (int64_t)d.R * d.C, KC_ = (int64_t)d.Kr * d.C, KH = (int64_t)d.Kr * d.hidden;
    const bool sub = d.Kr != d.R;
    int64_t o = 0;
    f.t = o; o += d.layout ? 0 : al(RC);
    f.a1 = o; o += al(RC);
    f.stats1 = o; o += al(2 * (int64_t)d.R);
    f.qkv = o; o += al(3 * RC);
    f.O = o; o += al(RC);
    f.Ok = o; o += sub ? al(KC_) : 0;
    f.tk = o; o += sub ? al(KC_) : 0;
    f.y1 = o; o += al(KC_);
    f.a2 = o; o += al(KC_);
    f.stats2 = o; o += al(2 * (int64_t)d.Kr);
    f.pre = o; o += al(KH);
    f.gact = o; o += al(KH);
    f.lse = o; o += al((int64_t)d.B * d.heads * d.N);
    f.total = o;
    return f;
}

// backward scratch: dh | da2 | dy1k | dOk | dy1, dO (stride > 1 only: on all token rows, dropped ones zero) | dqkv | da1 |
// dt (NCHW only) | LayerNorm parts | weight-gradient parts | bias parts
struct BwdLayout { int64_t dh, da2, dy1k, dOk, dy1, dO, dqkv, da1, dt, ln2, ln1, pq, po, p1, p2, bq, bo, b1, b2, total; };
BwdLayout bwd_layout(const WideDims& d) {
    BwdLayout b;
    const int64_t RC = (int64_t)d.R * d.C, KC_ = (int64_t)d.Kr * d.C, KH = (int64_t)d.Kr * d.hidden;
    const bool sub = d.Kr != d.R;
    int64_t o = 0;
    b.dh = o; o += al(KH);
    b.da2 = o; o += al(KC_);
    b.dy1k = o; o += al(KC_);
    b.dOk = o; o += al(KC_);
    b.dy1 = o; o += sub ? al(RC) : 0;
    b.dO = o; o += sub ? al(RC) : 0;
    b.dqkv = o; o += al(3 * RC);
    b.da1 = o; o += al(RC);
    b.dt = o; o += d.layout ? 0 : al(RC);
    b.ln2 = o; o += al((int64_t)((d.Kr + LNB - 1) / LNB) * 2 * d.C);
    b.ln1 = o; o += al((int64_t)((d.R + LNB - 1) / LNB) * 2 * d.C);
    b.pq = o; o += wg_part_floats(d.R, 3 * d.C, d.C);
    b.po = o; o += wg_part_floats(d.Kr, d.C, d.C);
    b.p1 = o; o += wg_part_floats(d.Kr, d.hidden, d.C);
    b.p2 = o; o += wg_part_floats(d.Kr, d.C, d.hidden);
    b.bq = o; o += cs_part_floats(d.R, 3 * d.C);
    b.bo = o; o += cs_part_floats(d.Kr, d.C);
    b.b1 = o; o += cs_part_floats(d.Kr, d.hidden);
    b.b2 = o; o += cs_part_floats(d.Kr, d.C);
    b.total = o;
    return b;
}

#define WIDE_CHECK(what) { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { ghn3_set_error("msa wide " what ": %s", hipGetErrorString(e_)); return GHN3_E_HIP; } }

int transpose_launch(float* dst, const float* src, int batches, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(wide_transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32, batches), dim3(NT), 0, s, dst, src, rows, cols);
    WIDE_CHECK("transpose");
    return GHN3_OK;
}
int rows_copy_launch(float* dst, const float* src, const WideDims& d, int scatter, hipStream_t s) {
    hipLaunchKernelGGL(wide_rows_copy_kernel, dim3(d.Kr), dim3(NT), 0, s, dst, src, d, scatter);
    WIDE_CHECK("rows copy");
    return GHN3_OK;
}
int ln_fwd_launch(const float* x, int rows, const WideDims& d, const float* g, const float* b, float* a, float* stats, hipStream_t s) {
    hipLaunchKernelGGL(wide_ln_fwd_kernel, dim3((rows + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, s, x, rows, d.C, d.eps, g, b, a, stats);
    WIDE_CHECK("layernorm");
    return GHN3_OK;
}
int ln_bwd_launch(const float* da, const float* x, const float* stats, const float* g, const float* res, float* dx, float* part,
                  int rows, int C, hipStream_t s) {
    hipLaunchKernelGGL(wide_ln_bwd_kernel, dim3((rows + LNB - 1) / LNB), dim3(NT), 0, s, da, x, stats, g, res, dx, part, rows, C);
    WIDE_CHECK("layernorm bwd");
    return GHN3_OK;
}
// the bias gradient db [Nout] = column sums of G: partials now, their sum with the other reductions
int colsum_launch(const float* G, int rows, int Nout, float* part, float* db, hipStream_t s, TnetRedProb* red, int* n_red) {
    const CsPlan p = cs_plan(rows);
    hipLaunchKernelGGL(wide_colsum_kernel, dim3((Nout + NT - 1) / NT, p.chunks), dim3(NT), 0, s, G, rows, Nout, p.per, part);
    WIDE_CHECK("bias gradient");
    red[(*n_red)++] = TnetRedProb{part, db, nullptr, p.chunks, Nout, Nout, Nout, 1};
    return GHN3_OK;
}

int wide_fwd(const WideDims& d, const float* x, const ghn3_msa_params& p, float* out, float* sc, hipStream_t s) {
    const FwdLayout f = fwd_layout(d);
    const bool sub = d.Kr != d.R;
    int rc;
    const float* t = x;
    if (!d.layout) {                                                   // NCHW [B][C][N] -> tokens [B][N][C]
        if ((rc = transpose_launch(sc + f.t, x, d.B, d.C, d.N, s))) return rc;
        t = sc + f.t;
    }
    if ((rc = ln_fwd_launch(t, d.R, d, p.ln1_w, p.ln1_b, sc + f.a1, sc + f.stats1, s))) return rc;
    if ((rc = linear_fwd("qkv", sc + f.a1, p.w_qkv, p.b_qkv, nullptr, sc + f.qkv, d.R, 3 * d.C, d.C, s))) return rc;
    if ((rc = ghn3_attn_wide_fwd(sc + f.O, sc + f.lse, sc + f.qkv, d.B, d.N, d.C, d.heads, s))) return rc;
    const float *Ok = sc + f.O, *tk = t;
    if (sub) {
        if ((rc = rows_copy_launch(sc + f.Ok, sc + f.O, d, 0, s))) return rc;
        if ((rc = rows_copy_launch(sc + f.tk, t, d, 0, s))) return rc;
        Ok = sc + f.Ok;
        tk = sc + f.tk;
    }
    if ((rc = linear_fwd("out projection", Ok, p.w_o, p.b_o, tk, sc + f.y1, d.Kr, d.C, d.C, s))) return rc;
    if ((rc = ln_fwd_launch(sc + f.y1, d.Kr, d, p.ln2_w, p.ln2_b, sc + f.a2, sc + f.stats2, s))) return rc;
    {
        const WGemm g{sc + f.a2, p.w1, sc + f.pre, d.Kr, d.hidden, d.C, d.C, d.C, d.hidden, (d.C + GK - 1) / GK * GK, 0,
                      p.b1, nullptr, nullptr, sc + f.gact};
        if ((rc = gemm_launch<false, false, EPI_GELU>("ff1", g, 1, s))) return rc;
    }
    return linear_fwd("ff2", sc + f.gact, p.w2, p.b2, sc + f.y1, out, d.Kr, d.C, d.hidden, s);
}

int wide_bwd(const WideDims& d, const float* dout, const float* x, const ghn3_msa_params& p, const float* fs, float* dx,
             const ghn3_msa_grads& g, float* sc, hipStream_t s) {
    const FwdLayout f = fwd_layout(d);
    const BwdLayout b = bwd_layout(d);
    const bool sub = d.Kr != d.R;
    int rc;
    const float* t = d.layout ? x : fs + f.t;
    const float* Ok = sub ? fs + f.Ok : fs + f.O;
    // feed-forward block
    if ((rc = linear_dgrad("ff2 dgrad", dout, p.w2, fs + f.pre, sc + b.dh, d.Kr, d.C, d.hidden, s))) return rc;
    if ((rc = linear_dgrad("ff1 dgrad", sc + b.dh, p.w1, nullptr, sc + b.da2, d.Kr, d.hidden, d.C, s))) return rc;
    if ((rc = ln_bwd_launch(sc + b.da2, fs + f.y1, fs + f.stats2, p.ln2_w, dout, sc + b.dy1k, sc + b.ln2, d.Kr, d.C, s))) return rc;
    // attention block
    if ((rc = linear_dgrad("out projection dgrad", sc + b.dy1k, p.w_o, nullptr, sc + b.dOk, d.Kr, d.C, d.C, s))) return rc;
    const float *dy1 = sc + b.dy1k, *dO = sc + b.dOk;
    if (sub) {                                                         // (dropped rows: no gradient reaches them through y)
        hipError_t e = hipMemsetAsync(sc + b.dy1, 0, (size_t)(b.dqkv - b.dy1) * sizeof(float), s);       // dy1, dO
        if (e != hipSuccess) { ghn3_set_error("msa wide bwd: hipMemsetAsync: %s", hipGetErrorString(e)); return GHN3_E_HIP; }
        if ((rc = rows_copy_launch(sc + b.dy1, sc + b.dy1k, d, 1, s))) return rc;
        if ((rc = rows_copy_launch(sc + b.dO, sc + b.dOk, d, 1, s))) return rc;
        dy1 = sc + b.dy1;
        dO = sc + b.dO;
    }
    if ((rc = ghn3_attn_wide_bwd(sc + b.dqkv, dO, fs + f.qkv, fs + f.lse, fs + f.O, d.B, d.N, d.C, d.heads, s))) return rc;
    if ((rc = linear_dgrad("qkv dgrad", sc + b.dqkv, p.w_qkv, nullptr, sc + b.da1, d.R, 3 * d.C, d.C, s))) return rc;
    float* dt = d.layout ? dx : sc + b.dt;
    if ((rc = ln_bwd_launch(sc + b.da1, t, fs + f.stats1, p.ln1_w, dy1, dt, sc + b.ln1, d.R, d.C, s))) return rc;
    if (!d.layout && (rc = transpose_launch(dx, dt, d.B, d.N, d.C, s))) return rc;
    // parameter gradients: dWqkv = dqkv^T a1, dWo = dy1^T O (kept rows), dW1 = dh^T a2, dW2 = dout^T gelu; biases: column sums
    TnetRedProb red[10];
    int n = 0;
    if ((rc = linear_wgrad("qkv wgrad", sc + b.dqkv, fs + f.a1, sc + b.pq, g.w_qkv, d.R, 3 * d.C, d.C, s, red, &n))) return rc;
    if ((rc = linear_wgrad("out projection wgrad", sc + b.dy1k, Ok, sc + b.po, g.w_o, d.Kr, d.C, d.C, s, red, &n))) return rc;
    if ((rc = linear_wgrad("ff1 wgrad", sc + b.dh, fs + f.a2, sc + b.p1, g.w1, d.Kr, d.hidden, d.C, s, red, &n))) return rc;
    if ((rc = linear_wgrad("ff2 wgrad", dout, fs + f.gact, sc + b.p2, g.w2, d.Kr, d.C, d.hidden, s, red, &n))) return rc;
    if (g.b_qkv && (rc = colsum_launch(sc + b.dqkv, d.R, 3 * d.C, sc + b.bq, g.b_qkv, s, red, &n))) return rc;
    if ((rc = colsum_launch(sc + b.dy1k, d.Kr, d.C, sc + b.bo, g.b_o, s, red, &n))) return rc;
    if ((rc = colsum_launch(sc + b.dh, d.Kr, d.hidden, sc + b.b1, g.b1, s, red, &n))) return rc;
    if ((rc = colsum_launch(dout, d.Kr, d.C, sc + b.b2, g.b2, s, red, &n))) return rc;
    red[n++] = TnetRedProb{sc + b.ln1, g.ln1_w, g.ln1_b, (d.R + LNB - 1) / LNB, 2 * d.C, d.C, d.C, 1};
    red[n++] = TnetRedProb{sc + b.ln2, g.ln2_w, g.ln2_b, (d.Kr + LNB - 1) / LNB, 2 * d.C, d.C, d.C, 1};
    for (int i = 0; i < n; i += TNET_RED_MAX)
        if ((rc = tnet_reduce_launch(red + i, std::min(TNET_RED_MAX, n - i), s))) return rc;
    return GHN3_OK;
}

// every pointer present; the ones read as float4 16-byte aligned
bool params_ok(const ghn3_msa_params* p, int has_qkv_bias) {
    return p && p->ln1_w && p->ln1_b && p->w_qkv && (!has_qkv_bias || p->b_qkv) && p->w_o && p->b_o && p->ln2_w && p->ln2_b &&
           p->w1 && p->b1 && p->w2 && p->b2 && a16(p->w_qkv) && a16(p->w_o) && a16(p->w1) && a16(p->w2);
}

}  // namespace

extern "C" int64_t ghn3_msa_wide_scratch_floats(const ghn3_msa_desc* desc, int backward) {
    WideDims d;
    const int rc = check_wide(desc, &d);
    if (rc) return rc;
    return backward ? bwd_layout(d).total : fwd_layout(d).total;
}

extern "C" int ghn3_msa_wide_fwd(const ghn3_msa_desc* desc, const float* x, const ghn3_msa_params* params, float* out,
                                 float* scratch, int save, void* stream) {
    (void)save;                              // (the forward is the same in both modes; the caller keeps the scratch or not)
    WideDims d;
    int rc = check_wide(desc, &d);
    if (rc) return rc;
    if (!x || !out || !scratch || !params_ok(params, desc->has_qkv_bias) || !a16(x) || !a16(out) || !a16(scratch)) {
        ghn3_set_error("msa wide fwd: null or misaligned pointer (x, out, scratch and the weight matrices need 16-byte alignment)");
        return GHN3_E_ARG;
    }
    ghn3_msa_params p = *params;
    if (!desc->has_qkv_bias) p.b_qkv = nullptr;
    return wide_fwd(d, x, p, out, scratch, (hipStream_t)stream);
}

extern "C" int ghn3_msa_wide_bwd(const ghn3_msa_desc* desc, const float* dout, const float* x, const ghn3_msa_params* params,
                                 const float* fwd_scratch, float* dx, const ghn3_msa_grads* grads, float* scratch, void* stream) {
    WideDims d;
    int rc = check_wide(desc, &d);
    if (rc) return rc;
    if (!dout || !x || !fwd_scratch || !dx || !scratch || !grads || !params_ok(params, desc->has_qkv_bias) || !a16(dout) ||
        !a16(x) || !a16(fwd_scratch) || !a16(dx) || !a16(scratch)) {
        ghn3_set_error("msa wide bwd: null or misaligned pointer");
        return GHN3_E_ARG;
    }
    const ghn3_msa_grads& g = *grads;
    if (!g.ln1_w || !g.ln1_b || !g.w_qkv || (desc->has_qkv_bias && !g.b_qkv) || !g.w_o || !g.b_o || !g.ln2_w || !g.ln2_b ||
        !g.w1 || !g.b1 || !g.w2 || !g.b2) {
        ghn3_set_error("msa wide bwd: null gradient pointer");
        return GHN3_E_ARG;
    }
    ghn3_msa_params p = *params;
    ghn3_msa_grads gg = g;
    if (!desc->has_qkv_bias) { p.b_qkv = nullptr; gg.b_qkv = nullptr; }
    return wide_bwd(d, dout, x, p, fwd_scratch, dx, gg, scratch, (hipStream_t)stream);
}
