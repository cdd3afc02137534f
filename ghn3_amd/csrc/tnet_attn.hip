// Target-network layers: the attention core of the `msa` op without a saved N x N matrix ("lean" attention).
//
// Plain multi-head self-attention on the qkv [B N][3 C] layout of ghn3_attn_fwd (attention.hip): no bias, no padding (every
// sequence has N tokens), scale = 1 / sqrt(d), d = C / heads <= 32, C % 4 == 0, 1 <= N <= 4096.  The forward keeps one float
// per query row, lse_i = ln sum_j exp(scale q_i . k_j); the backward recomputes P = exp(scale S - lse) from Q, K and lse
// instead of reading P [B][heads][N][N] back: the saved state is O(N), not O(N^2).
//
// Every product runs on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate) with the tile orientation of
// attention.hip: a score-shaped 32 x 32 tile has the OWNED index (the workgroup's 32 queries, or its 32 keys) on the lane and
// the streamed index in the 16 accumulator registers, so the softmax is a per-lane loop and the tile is already the B operand
// of the product that follows it.  Four waves split the 32-wide tiles of the streamed dimension (operands straight from memory:
// a head slice is up to 4096 x 32 floats per operand and does not fit in LDS) and sum their partial outputs through LDS in wave
// order.  No float atomics: reruns are bit-identical.
//
//   forward   grid (ceil(N / 32), heads, B).  Two passes over the key tiles, as attn_fwd_stream_kernel: pass 1 keeps a running
//             (max, sum) per query -- rescaled exactly whenever the maximum moves --, pass 2 recomputes the scores, normalises
//             and accumulates O^T = V^T P^T.  Writes out and, when asked, lse = max + ln(sum).
//   backward  grid (2 ceil(N / 32), heads, B), the two roles of attn_bwd_kernel.  Row workgroups own 32 queries and produce dQ
//             (S^T, dP^T, dQ^T: 3 products per tile); column workgroups own 32 keys and produce dK and dV (S, dP, dV^T, dK^T: 4
//             products).  The row constants -lse_i and -delta_i (delta_i = sum_e dO_ie O_ie) are the INITIAL accumulators of S
//             and dP, and q enters pre-multiplied by the scale, so P = exp(acc) and dS = P . acc' need no further arithmetic.
//             delta is recomputed from the dO and O rows the tile loads anyway.  Every element of dqkv is written.
// The forward forms its scores from the same pre-scaled q, so the backward's P sums to one to rounding.

#include <math.h>
#include "tnet_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int LEAN_NW = 4;                  // waves per workgroup
constexpr int LEAN_DMAX = 32, LEAN_NMAX = 4096;

// row of accumulator register r in the 32 x 32 C/D layout (column = lane & 31)
__device__ __forceinline__ int acc_row(int r, int lhi) { return (r & 3) + 8 * (r >> 2) + 4 * lhi; }
__device__ __forceinline__ f32x16 splat16(float v) {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = v;
    return z;
}

// Row operand (lane & 31 = matrix row `row` of X, MFMA step s <-> k = 2 s + lhi): x[s] = mul X[row][2 s + lhi], zero for
// k >= d or row >= n_rows.  Every load is unconditional (row and offsets clamped, the value selected afterwards), so the loads of
// a tile's operands are all in flight together.  vec: d % 4 == 0 and 16-byte rows.
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

// Column operand (lane & 31 = head column e, MFMA step s <-> row row0 + acc_row(s, lhi) of X): zero for e >= d or rows >= n_rows
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

// Sum of the waves' 32 x 32 partial tiles through LDS, in wave order; wave w returns register group w of the total: the four
// consecutive head columns e = 8 w + 4 lhi + c of matrix column lane & 31.
__device__ __forceinline__ f32x4 reduce_waves(float* red /* [LEAN_NW][16][64] */, const f32x16& part, int w, int lane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(w * 16 + r) * 64 + lane] = part[r];
    __syncthreads();
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int r = 4 * w + c;
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < LEAN_NW; ++q) t += red[(16 * q + r) * 64 + lane];
        o[c] = t;
    }
    return o;
}

// dst[e0 .. e0 + 3] = v (only e < d)
__device__ __forceinline__ void store4(float* __restrict__ dst, int e0, int d, bool vec, f32x4 v) {
    if (vec && e0 + 3 < d) {
        *reinterpret_cast<f32x4*>(dst + e0) = v;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (e0 + c < d) dst[e0 + c] = v[c];
    }
}

// S^T of key tile j0 for this lane's query (qb pre-scaled): register r <-> key j0 + acc_row(r, lhi); keys >= N: -inf
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

// ------------------------------------------------------------------------------------------------ forward
template <int KS>
__global__ __launch_bounds__(64 * LEAN_NW, 2) void attn_lean_fwd_kernel(float* __restrict__ out, float* __restrict__ lse,
                                                                        const float* __restrict__ qkv, int N, int C, int H,
                                                                        float scale, int vec16) {
    __shared__ float red[LEAN_NW * 16 * 64];
    __shared__ float red_m[LEAN_NW][32], red_l[LEAN_NW][32];
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

    // pass 1: running maximum and sum of this lane's keys (every tile has a key below N, so its maximum is finite)
    float mx = -INFINITY, sum = 0.f;
    for (int t = w; t < NB; t += LEAN_NW) {
        const f32x16 sc = score_tile<KS>(base + C, qb, t * 32, N, C, d, l31, lhi, vec);
        float tm = mx;
#pragma unroll
        for (int r = 0; r < 16; ++r) tm = fmaxf(tm, sc[r]);
        float acc = sum * expf(mx - tm);                         // (mx = -inf on the first tile: exp(-inf) = 0)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc += expf(sc[r] - tm);
        sum = acc;
        mx = tm;
    }
    {   // the two half-waves of a query hold different keys
        const float m2 = __shfl_xor(mx, 32, 64), s2 = __shfl_xor(sum, 32, 64);
        const float mn = fmaxf(mx, m2);
        sum = (mx > -INFINITY ? sum * expf(mx - mn) : 0.f) + (m2 > -INFINITY ? s2 * expf(m2 - mn) : 0.f);
        mx = mn;
    }
    if (lhi == 0) { red_m[w][l31] = mx; red_l[w][l31] = sum; }
    __syncthreads();
    float gm = red_m[0][l31];                                    // (wave 0 always has a tile)
#pragma unroll
    for (int k = 1; k < LEAN_NW; ++k) gm = fmaxf(gm, red_m[k][l31]);
    float gl = 0.f;
#pragma unroll
    for (int k = 0; k < LEAN_NW; ++k)
        if (red_m[k][l31] > -INFINITY) gl += red_l[k][l31] * expf(red_m[k][l31] - gm);
    const float inv = 1.f / gl;
    if (lse && w == 0 && lhi == 0 && qi < N) lse[bh + qi] = gm + logf(gl);

    // pass 2: P^T = exp(S^T - max) / sum, O^T += V^T P^T
    f32x16 O = splat16(0.f);
    for (int t = w; t < NB; t += LEAN_NW) {
        const int j0 = t * 32;
        f32x16 sc = score_tile<KS>(base + C, qb, j0, N, C, d, l31, lhi, vec);
        float va[16];
        col_operand(base + 2 * C, j0, N, (size_t)3 * C, l31, d, lhi, va);
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = expf(sc[r] - gm) * inv;
        O = mfma_cols(va, sc, O);
    }
    const f32x4 o = reduce_waves(red, O, w, lane);
    if (qi < N) store4(out + ((size_t)b * N + qi) * C + h * d, 8 * w + 4 * lhi, d, vec, o);
}

// ------------------------------------------------------------------------------------------------ backward
template <int KS>
__global__ __launch_bounds__(64 * LEAN_NW, 2) void attn_lean_bwd_kernel(float* __restrict__ dqkv, const float* __restrict__ dO,
                                                                        const float* __restrict__ qkv,
                                                                        const float* __restrict__ lse,
                                                                        const float* __restrict__ Oin, int N, int C, int H,
                                                                        float scale, int vec16) {
    __shared__ float red[LEAN_NW * 16 * 64];
    __shared__ float dl[LEAN_NW][32], ll[LEAN_NW][32];
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
        float qb[KS], gb[KS], ob[KS];
        row_operand<KS>(base, qi, N, s3, d, lhi, vec, scale, qb);
        row_operand<KS>(dOb, qi, N, s1, d, lhi, vec, 1.f, gb);
        row_operand<KS>(Ob, qi, N, s1, d, lhi, vec, 1.f, ob);
        const float lq = lb[min(qi, N - 1)];
        float delta = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) delta += gb[s] * ob[s];
        delta += __shfl_xor(delta, 32, 64);
        const f32x16 s_init = splat16(qok ? -lq : 0.f), dp_init = splat16(-delta);
        f32x16 dQ = splat16(0.f);
        for (int t = w; t < NB; t += LEAN_NW) {
            const int j0 = t * 32;
            float ka[KS], va[KS], kc[16];
            row_operand<KS>(base + C, j0 + l31, N, s3, d, lhi, vec, 1.f, ka);
            row_operand<KS>(base + 2 * C, j0 + l31, N, s3, d, lhi, vec, 1.f, va);
            col_operand(base + C, j0, N, s3, l31, d, lhi, kc);
            const f32x16 sc = mfma_rows<KS>(ka, qb, s_init);           // scale S^T - lse = scale K Q^T - lse
            f32x16 ds = mfma_rows<KS>(va, gb, dp_init);                // dP^T - delta = V dO^T - delta
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = (qok && j0 + acc_row(r, lhi) < N) ? expf(sc[r]) : 0.f;
                ds[r] = p * ds[r];
            }
            dQ = mfma_cols(kc, ds, dQ);                                // dQ^T += K^T dS^T
        }
        f32x4 o = reduce_waves(red, dQ, w, lane);
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] *= scale;
        if (qok) store4(dqkv + ((size_t)b * N + qi) * s3 + h * d, 8 * w + 4 * lhi, d, vec, o);
    } else {
        // ---------------- column role: lane = key kj, accumulator registers = queries ----------------
        const int kj = (blockIdx.x - NB) * 32 + l31;
        const bool kok = kj < N;
        float kb[KS], vb[KS];
        row_operand<KS>(base + C, kj, N, s3, d, lhi, vec, 1.f, kb);
        row_operand<KS>(base + 2 * C, kj, N, s3, d, lhi, vec, 1.f, vb);
        f32x16 dV = splat16(0.f), dK = splat16(0.f);
        for (int t = w; t < NB; t += LEAN_NW) {
            const int q0 = t * 32, qrow = q0 + l31;
            float qa[KS], ga[KS], oa[KS], gc[16], qc[16];
            row_operand<KS>(base, qrow, N, s3, d, lhi, vec, scale, qa);
            row_operand<KS>(dOb, qrow, N, s1, d, lhi, vec, 1.f, ga);
            row_operand<KS>(Ob, qrow, N, s1, d, lhi, vec, 1.f, oa);
            col_operand(dOb, q0, N, s1, l31, d, lhi, gc);
            col_operand(base, q0, N, s3, l31, d, lhi, qc);
            const float lq = lb[min(qrow, N - 1)];
            float dpart = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) dpart += ga[s] * oa[s];
            dpart += __shfl_xor(dpart, 32, 64);
            // wave-private hand-off of the row constants: lane (query) -> accumulator register index
            if (lhi == 0) { dl[w][l31] = -dpart; ll[w][l31] = qrow < N ? -lq : 0.f; }
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            f32x16 sc, ds;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sc[r] = ll[w][acc_row(r, lhi)]; ds[r] = dl[w][acc_row(r, lhi)]; }
            sc = mfma_rows<KS>(qa, kb, sc);                            // scale S - lse   (rows = queries, lane = key)
            ds = mfma_rows<KS>(ga, vb, ds);                            // dP - delta = dO V^T - delta
            f32x16 p;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = (kok && q0 + acc_row(r, lhi) < N) ? expf(sc[r]) : 0.f;
                ds[r] = p[r] * ds[r];
            }
            __builtin_amdgcn_wave_barrier();                           // (the next tile rewrites dl and ll)
            dV = mfma_cols(gc, p, dV);                                 // dV^T += dO^T P
            dK = mfma_cols(qc, ds, dK);                                // dK^T += Q^T dS
        }
        const f32x4 ov = reduce_waves(red, dV, w, lane);
        __syncthreads();                                               // (one exchange buffer for both reductions)
        f32x4 ok = reduce_waves(red, dK, w, lane);
#pragma unroll
        for (int c = 0; c < 4; ++c) ok[c] *= scale;
        if (kok) {
            float* row = dqkv + ((size_t)b * N + kj) * s3 + h * d;
            store4(row + 2 * C, 8 * w + 4 * lhi, d, vec, ov);
            store4(row + C, 8 * w + 4 * lhi, d, vec, ok);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
int check_dims(const char* what, int B, int N, int C, int H) {
    if (B <= 0 || B > 65535 || H <= 0 || H > 65535 || C <= 0 || C % 4 || C % H || C / H > LEAN_DMAX) {
        ghn3_set_error("%s: needs 1 <= B, heads <= 65535, C %% 4 == 0, C %% heads == 0 and head dim <= %d (B %d, C %d, heads %d)",
                       what, LEAN_DMAX, B, C, H);
        return GHN3_E_LIMIT;
    }
    if (N <= 0 || N > LEAN_NMAX) { ghn3_set_error("%s: N = %d outside [1, %d]", what, N, LEAN_NMAX); return GHN3_E_LIMIT; }
    return GHN3_OK;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int ghn3_attn_lean_fwd(float* out, float* lse, const float* qkv, int B, int N, int C, int heads, void* stream) {
    int rc = check_dims("lean attention fwd", B, N, C, heads);
    if (rc) return rc;
    if (!out || !qkv) { ghn3_set_error("lean attention fwd: null pointer"); return GHN3_E_ARG; }
    const int d = C / heads, nb = (N + 31) / 32;
    const float scale = 1.0f / sqrtf((float)d);
    const int vec = aligned16(out) && aligned16(qkv);
    auto fn = d <= 4 ? attn_lean_fwd_kernel<2> : d <= 8 ? attn_lean_fwd_kernel<4> : d <= 16 ? attn_lean_fwd_kernel<8>
              : d <= 24 ? attn_lean_fwd_kernel<12> : attn_lean_fwd_kernel<16>;
    hipLaunchKernelGGL(fn, dim3(nb, heads, B), dim3(64 * LEAN_NW), 0, (hipStream_t)stream, out, lse, qkv, N, C, heads, scale, vec);
    TNET_LAUNCH_CHECK("lean attention fwd");
    return GHN3_OK;
}

extern "C" int ghn3_attn_lean_bwd(float* dqkv, const float* dO, const float* qkv, const float* lse, const float* O, int B, int N,
                                  int C, int heads, void* stream) {
    int rc = check_dims("lean attention bwd", B, N, C, heads);
    if (rc) return rc;
    if (!dqkv || !dO || !qkv || !lse || !O) {
        ghn3_set_error("lean attention bwd: null pointer (needs the forward's lse and output)");
        return GHN3_E_ARG;
    }
    const int d = C / heads, nb = (N + 31) / 32;
    const float scale = 1.0f / sqrtf((float)d);
    const int vec = aligned16(dqkv) && aligned16(dO) && aligned16(qkv) && aligned16(O);
    auto fn = d <= 4 ? attn_lean_bwd_kernel<2> : d <= 8 ? attn_lean_bwd_kernel<4> : d <= 16 ? attn_lean_bwd_kernel<8>
              : d <= 24 ? attn_lean_bwd_kernel<12> : attn_lean_bwd_kernel<16>;
    hipLaunchKernelGGL(fn, dim3(2 * nb, heads, B), dim3(64 * LEAN_NW), 0, (hipStream_t)stream, dqkv, dO, qkv, lse, O, N, C, heads,
                       scale, vec);
    TNET_LAUNCH_CHECK("lean attention bwd");
    return GHN3_OK;
}
