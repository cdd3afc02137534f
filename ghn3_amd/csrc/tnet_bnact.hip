// A BatchNorm [+ ReLU] that stands alone -- no convolution in front of it -- on the op family's storage (include/ghn3_hip.h,
// "stand-alone BatchNorm"): the leading layers of a DenseNet's dense layer and of a pre-activation residual block.  x is
// [P = N H W][C] fp32 (NHWC); plain fp32 and bandwidth-bound, so the launches are few and every pass of activation size is
// needed: batch statistics read x twice and write out once (2 launches), their backward reads dout and x twice and writes dx
// once (2 launches); frozen statistics take one launch forward and two backward (the second one is of parameter size).
//
// Geometry.  A workgroup is 256 threads = (channel quad) x (row lane) over a CHANNEL BLOCK of 64 channels -- 16 quads x 16 row
// lanes; a layer narrower than 64 channels has C / 4 quads and 256 / (C / 4) row lanes --, so one lane moves 16 bytes and 16
// neighbouring lanes move 256 contiguous bytes of a row.  grid.y = min(channel blocks, 16): up to 1024 channels every block has a
// workgroup column of its own, wider layers loop (block y, y + 16, ...).  grid.x = row chunks (the two partial kernels) or row
// blocks (the two streaming kernels); both are pure functions of (P, C) (plan_of), so a result never depends on the device.
//
// Statistics: per row chunk and channel (mean, M2), Chan-combined in a fixed order -- the family's rule, never sum / sum of
// squares.  Inside a chunk a thread sums x - s and (x - s)^2 with s = ITS OWN first element: s lies within the channel's spread
// of the mean, so nothing cancels for a channel whose mean is far from zero, and a constant channel gives M2 = 0 exactly.  The row
// lanes are combined in lane order through LDS.  The second kernel of each direction has no launch in front of it that would
// combine the chunks: EVERY workgroup combines the partials of its own channel block, all in the same order (4 chunk lanes over
// chunks l, l + 4, ..., then the lanes in order), so all of them hold the same bits, and the workgroups of row block 0 write
// the statistics (forward) or dgamma / dbeta (backward).  No atomics anywhere.
//
// The ReLU mask of the backward is RECOMPUTED from x -- y = fma((x - mean) rstd, gamma, beta) with explicit single-rounding
// intrinsics (bnact_pre), the very instructions the forward used, so the bits of y and the mask 1[y > 0] are the forward's --
// where dout is first read.  Neither out nor anything else of activation size is saved besides x.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>

#include "tnet_common.h"

namespace {

constexpr int BA_THREADS = 256;
constexpr int BA_CBW = 64;              // channels of a channel block
constexpr int BA_GRID_Y = 16;           // channel blocks side by side in a grid: wider layers (C > 1024) loop
constexpr int BA_TILE = 64;             // a row chunk is a multiple of this many rows
constexpr int BA_LANES = 4;             // chunk lanes of the combination in the streaming kernels
constexpr int BA_MAX_C = 16384;
constexpr int64_t BA_MAX_ELEMS = (int64_t)1 << 31;

struct Plan {
    int ncb, gy;                        // channel blocks, grid.y
    int rows_chunk, n_chunks;           // the partial kernels: rows per chunk (a multiple of BA_TILE), chunks
    int rows_rb, n_rb;                  // the streaming kernels: rows per row block (a multiple of 16), row blocks
};

// About 512 workgroups for the partial kernels, but no more than 128 chunks (every workgroup of the streaming kernel reads all
// partials of its channel block) and, for the same reason, row blocks of at least 2 n_chunks rows.
Plan plan_of(int P, int C) {
    Plan pl;
    pl.ncb = (C + BA_CBW - 1) / BA_CBW;
    pl.gy = std::min(pl.ncb, BA_GRID_Y);
    const int tiles = (P + BA_TILE - 1) / BA_TILE;
    const int max_chunks = std::max(32, std::min(128, 512 / pl.gy));
    pl.rows_chunk = (tiles + max_chunks - 1) / max_chunks * BA_TILE;
    pl.n_chunks = (P + pl.rows_chunk - 1) / pl.rows_chunk;
    const int max_rb = 2048 / pl.gy;
    const int rows = std::max(std::max(BA_TILE, 2 * pl.n_chunks), (P + max_rb - 1) / max_rb);
    pl.rows_rb = (rows + 15) / 16 * 16;
    pl.n_rb = (P + pl.rows_rb - 1) / pl.rows_rb;
    return pl;
}

// (n, mean, M2) += (nb, mb, Mb), Chan et al.; an empty side changes nothing, and an empty left side takes the right one as it is
__device__ __forceinline__ void chan(float& n, float& mean, float& M2, float nb, float mb, float Mb) {
    if (nb <= 0.f) return;
    if (n <= 0.f) { n = nb; mean = mb; M2 = Mb; return; }
    const float nn = n + nb, dl = mb - mean;
    mean += dl * nb / nn;
    M2 += Mb + dl * dl * n * nb / nn;
    n = nn;
}

// the pre-activation, one rounding per step in this order in every kernel: the backward's mask is the forward's
__device__ __forceinline__ float bnact_pre(float x, float mu, float rs, float ga, float be) {
    return __fmaf_rn(__fmul_rn(__fsub_rn(x, mu), rs), ga, be);
}

struct Lanes {                          // the thread geometry of a workgroup
    int nq, ng, q, g;
};
__device__ __forceinline__ Lanes lanes_of(int C) {
    Lanes l;
    l.nq = min(BA_CBW / 4, C / 4);
    l.ng = BA_THREADS / l.nq;
    l.q = threadIdx.x % l.nq;
    l.g = threadIdx.x / l.nq;
    return l;
}

// ---- forward, launch 1: part[chunk][0][c] = mean, part[chunk][1][c] = M2 of the chunk's rows ----------------------------------
__global__ __launch_bounds__(BA_THREADS) void tnet_bnact_stats_partial_kernel(const float* __restrict__ x, float* __restrict__ part,
                                                                              int P, int C, int rows_chunk) {
    __shared__ float sn[4 * BA_THREADS], sm[4 * BA_THREADS], s2[4 * BA_THREADS];        // [row lane][channel of the block]
    const Lanes l = lanes_of(C);
    const int W = 4 * l.nq, ncb = (C + BA_CBW - 1) / BA_CBW;
    const int64_t r0 = (int64_t)blockIdx.x * rows_chunk, r1 = min((int64_t)P, r0 + rows_chunk);
    for (int cb = blockIdx.y; cb < ncb; cb += gridDim.y) {
        const int c = cb * BA_CBW + 4 * l.q;
        if (l.g < l.ng) {
            float n = 0.f;
            f32x4 sh = {0.f, 0.f, 0.f, 0.f}, a1 = sh, a2 = sh;
            int64_t p = r0 + l.g;
            if (c < C && p < r1) {
                sh = *reinterpret_cast<const f32x4*>(x + p * C + c);
                n = 1.f;
#pragma unroll 4
                for (p += l.ng; p < r1; p += l.ng) {
                    const f32x4 d = *reinterpret_cast<const f32x4*>(x + p * C + c) - sh;
                    a1 += d;
                    a2 += d * d;
                    n += 1.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = l.g * W + 4 * l.q + e;
                sn[i] = n;
                sm[i] = n > 0.f ? sh[e] + a1[e] / n : 0.f;
                s2[i] = n > 0.f ? fmaxf(a2[e] - a1[e] * a1[e] / n, 0.f) : 0.f;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < W && cb * BA_CBW + (int)threadIdx.x < C) {
            float n = 0.f, mean = 0.f, M2 = 0.f;
            for (int g = 0; g < l.ng; ++g) chan(n, mean, M2, sn[g * W + threadIdx.x], sm[g * W + threadIdx.x], s2[g * W + threadIdx.x]);
            const int cc = cb * BA_CBW + threadIdx.x;
            part[((int64_t)blockIdx.x * 2) * C + cc] = mean;
            part[((int64_t)blockIdx.x * 2 + 1) * C + cc] = M2;
        }
        __syncthreads();
    }
}

// what the streaming kernels keep in LDS per channel of the block
struct BlockConsts {
    float mu[BA_CBW], rs[BA_CBW], ga[BA_CBW], be[BA_CBW], a[BA_CBW], b[BA_CBW];
};

// ---- forward, launch 2 (batch statistics) / the only launch (frozen) ----------------------------------------------------------
// FROZEN: mean_in / var_in [C] are the statistics; else they come from part, and row block 0 writes stats [3 C] = mean, rstd,
// biased variance (the layout of ghn3_conv_bn_fwd).
template <bool FROZEN>
__global__ __launch_bounds__(BA_THREADS) void tnet_bnact_apply_kernel(const float* __restrict__ x, const float* __restrict__ part,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      const float* __restrict__ mean_in, const float* __restrict__ var_in,
                                                                      float* __restrict__ out, float* __restrict__ stats, int P, int C,
                                                                      int relu, float eps, int rows_chunk, int n_chunks, int rows_rb) {
    __shared__ float cn[BA_LANES][BA_CBW], cm[BA_LANES][BA_CBW], c2[BA_LANES][BA_CBW];
    __shared__ __attribute__((aligned(16))) BlockConsts k;
    const Lanes l = lanes_of(C);
    const int ncb = (C + BA_CBW - 1) / BA_CBW;
    const int ch = threadIdx.x % BA_CBW, lane = threadIdx.x / BA_CBW;
    const int64_t r0 = (int64_t)blockIdx.x * rows_rb, r1 = min((int64_t)P, r0 + rows_rb);
    for (int cb = blockIdx.y; cb < ncb; cb += gridDim.y) {
        const int cc = cb * BA_CBW + ch;
        if (!FROZEN) {
            float n = 0.f, mean = 0.f, M2 = 0.f;
            if (cc < C)
                for (int t = lane; t < n_chunks; t += BA_LANES)
                    chan(n, mean, M2, (float)min((int64_t)rows_chunk, (int64_t)P - (int64_t)t * rows_chunk), part[((int64_t)t * 2) * C + cc],
                         part[((int64_t)t * 2 + 1) * C + cc]);
            cn[lane][ch] = n; cm[lane][ch] = mean; c2[lane][ch] = M2;
            __syncthreads();
        }
        if (lane == 0) {
            float mean = 0.f, rstd = 0.f, ga = 0.f, be = 0.f;
            if (cc < C) {
                ga = gamma[cc];
                be = beta[cc];
                if (FROZEN) {
                    mean = mean_in[cc];
                    rstd = 1.f / sqrtf(var_in[cc] + eps);
                } else {
                    float n = cn[0][ch], M2 = c2[0][ch];
                    mean = cm[0][ch];
                    for (int j = 1; j < BA_LANES; ++j) chan(n, mean, M2, cn[j][ch], cm[j][ch], c2[j][ch]);
                    const float var = M2 / n;
                    rstd = 1.f / sqrtf(var + eps);
                    if (blockIdx.x == 0) {
                        stats[cc] = mean;
                        stats[C + cc] = rstd;
                        stats[2 * C + cc] = var;
                    }
                }
            }
            k.mu[ch] = mean; k.rs[ch] = rstd; k.ga[ch] = ga; k.be[ch] = be;
        }
        __syncthreads();
        const int c = cb * BA_CBW + 4 * l.q;
        if (l.g < l.ng && c < C) {
            const f32x4 mu = *reinterpret_cast<const f32x4*>(k.mu + 4 * l.q), rs = *reinterpret_cast<const f32x4*>(k.rs + 4 * l.q);
            const f32x4 ga = *reinterpret_cast<const f32x4*>(k.ga + 4 * l.q), be = *reinterpret_cast<const f32x4*>(k.be + 4 * l.q);
#pragma unroll 4
            for (int64_t p = r0 + l.g; p < r1; p += l.ng) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + p * C + c);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float y = bnact_pre(v[e], mu[e], rs[e], ga[e], be[e]);
                    o[e] = (relu && y <= 0.f) ? 0.f : y;
                }
                *reinterpret_cast<f32x4*>(out + p * C + c) = o;
            }
        }
        __syncthreads();
    }
}

// (mean, rstd, gamma, beta) of the channel block into LDS for the backward kernels: `stats` [3 C] of the forward, or
// (mean_in, var_in) of a frozen layer
template <bool FROZEN>
__device__ __forceinline__ void load_consts(BlockConsts& k, int cb, int C, const float* stats, const float* mean_in, const float* var_in,
                                            const float* gamma, const float* beta, float eps) {
    if ((int)threadIdx.x < BA_CBW) {
        const int ch = threadIdx.x, cc = cb * BA_CBW + ch;
        float mean = 0.f, rstd = 0.f, ga = 0.f, be = 0.f;
        if (cc < C) {
            ga = gamma[cc];
            be = beta[cc];
            mean = FROZEN ? mean_in[cc] : stats[cc];
            rstd = FROZEN ? 1.f / sqrtf(var_in[cc] + eps) : stats[C + cc];
        }
        k.mu[ch] = mean; k.rs[ch] = rstd; k.ga[ch] = ga; k.be[ch] = be;
    }
}

// ---- backward, launch 1: part[chunk][0][c] = sum g, part[chunk][1][c] = sum g xhat, g = dout 1[y > 0] (relu) or dout ----------
// FROZEN: dx = g gamma rstd does not depend on the sums and is written here as well.
template <bool FROZEN>
__global__ __launch_bounds__(BA_THREADS) void tnet_bnact_bwd_partial_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                                            const float* __restrict__ stats,
                                                                            const float* __restrict__ mean_in, const float* __restrict__ var_in,
                                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                            float* __restrict__ part, float* __restrict__ dx, int P, int C,
                                                                            int relu, float eps, int rows_chunk) {
    __shared__ float r1s[4 * BA_THREADS], r2s[4 * BA_THREADS];                             // [row lane][channel of the block]
    __shared__ __attribute__((aligned(16))) BlockConsts k;
    const Lanes l = lanes_of(C);
    const int W = 4 * l.nq, ncb = (C + BA_CBW - 1) / BA_CBW;
    const int64_t r0 = (int64_t)blockIdx.x * rows_chunk, r1 = min((int64_t)P, r0 + rows_chunk);
    for (int cb = blockIdx.y; cb < ncb; cb += gridDim.y) {
        load_consts<FROZEN>(k, cb, C, stats, mean_in, var_in, gamma, beta, eps);
        __syncthreads();
        const int c = cb * BA_CBW + 4 * l.q;
        if (l.g < l.ng) {
            f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
            if (c < C) {
                const f32x4 mu = *reinterpret_cast<const f32x4*>(k.mu + 4 * l.q), rs = *reinterpret_cast<const f32x4*>(k.rs + 4 * l.q);
                const f32x4 ga = *reinterpret_cast<const f32x4*>(k.ga + 4 * l.q), be = *reinterpret_cast<const f32x4*>(k.be + 4 * l.q);
#pragma unroll 4
                for (int64_t p = r0 + l.g; p < r1; p += l.ng) {
                    const f32x4 gd = *reinterpret_cast<const f32x4*>(dout + p * C + c);
                    const f32x4 v = *reinterpret_cast<const f32x4*>(x + p * C + c);
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float g = (relu && !(bnact_pre(v[e], mu[e], rs[e], ga[e], be[e]) > 0.f)) ? 0.f : gd[e];
                        s1[e] += g;
                        s2[e] += g * ((v[e] - mu[e]) * rs[e]);
                        o[e] = g * ga[e] * rs[e];
                    }
                    if (FROZEN) *reinterpret_cast<f32x4*>(dx + p * C + c) = o;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                r1s[l.g * W + 4 * l.q + e] = s1[e];
                r2s[l.g * W + 4 * l.q + e] = s2[e];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < W && cb * BA_CBW + (int)threadIdx.x < C) {
            float t1 = 0.f, t2 = 0.f;
            for (int g = 0; g < l.ng; ++g) { t1 += r1s[g * W + threadIdx.x]; t2 += r2s[g * W + threadIdx.x]; }
            const int cc = cb * BA_CBW + threadIdx.x;
            part[((int64_t)blockIdx.x * 2) * C + cc] = t1;
            part[((int64_t)blockIdx.x * 2 + 1) * C + cc] = t2;
        }
        __syncthreads();
    }
}

// ---- backward, launch 2 (batch statistics): dx = gamma rstd (g - mean(g) - xhat mean(g xhat)); row block 0 writes dbeta =
// sum g and dgamma = sum g xhat --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BA_THREADS) void tnet_bnact_dx_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                                   const float* __restrict__ stats, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, const float* __restrict__ part,
                                                                   float* __restrict__ dx, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta, int P, int C, int relu, int n_chunks,
                                                                   int rows_rb) {
    __shared__ float c1[BA_LANES][BA_CBW], c2[BA_LANES][BA_CBW];
    __shared__ __attribute__((aligned(16))) BlockConsts k;
    const Lanes l = lanes_of(C);
    const int ncb = (C + BA_CBW - 1) / BA_CBW;
    const int ch = threadIdx.x % BA_CBW, lane = threadIdx.x / BA_CBW;
    const int64_t r0 = (int64_t)blockIdx.x * rows_rb, r1 = min((int64_t)P, r0 + rows_rb);
    const float inv_p = 1.f / (float)P;
    for (int cb = blockIdx.y; cb < ncb; cb += gridDim.y) {
        const int cc = cb * BA_CBW + ch;
        float t1 = 0.f, t2 = 0.f;
        if (cc < C)
            for (int t = lane; t < n_chunks; t += BA_LANES) {
                t1 += part[((int64_t)t * 2) * C + cc];
                t2 += part[((int64_t)t * 2 + 1) * C + cc];
            }
        c1[lane][ch] = t1; c2[lane][ch] = t2;
        load_consts<false>(k, cb, C, stats, nullptr, nullptr, gamma, beta, 0.f);
        __syncthreads();
        if (lane == 0) {
            for (int j = 1; j < BA_LANES; ++j) { t1 += c1[j][ch]; t2 += c2[j][ch]; }
            if (cc < C && blockIdx.x == 0) {
                dbeta[cc] = t1;
                dgamma[cc] = t2;
            }
            k.a[ch] = t1 * inv_p;
            k.b[ch] = t2 * inv_p;
        }
        __syncthreads();
        const int c = cb * BA_CBW + 4 * l.q;
        if (l.g < l.ng && c < C) {
            const f32x4 mu = *reinterpret_cast<const f32x4*>(k.mu + 4 * l.q), rs = *reinterpret_cast<const f32x4*>(k.rs + 4 * l.q);
            const f32x4 ga = *reinterpret_cast<const f32x4*>(k.ga + 4 * l.q), be = *reinterpret_cast<const f32x4*>(k.be + 4 * l.q);
            const f32x4 ma = *reinterpret_cast<const f32x4*>(k.a + 4 * l.q), mb = *reinterpret_cast<const f32x4*>(k.b + 4 * l.q);
#pragma unroll 4
            for (int64_t p = r0 + l.g; p < r1; p += l.ng) {
                const f32x4 gd = *reinterpret_cast<const f32x4*>(dout + p * C + c);
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + p * C + c);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g = (relu && !(bnact_pre(v[e], mu[e], rs[e], ga[e], be[e]) > 0.f)) ? 0.f : gd[e];
                    const float xh = (v[e] - mu[e]) * rs[e];
                    o[e] = ga[e] * rs[e] * (g - ma[e] - xh * mb[e]);
                }
                *reinterpret_cast<f32x4*>(dx + p * C + c) = o;
            }
        }
        __syncthreads();
    }
}

// ---- frozen backward, launch 2: dbeta / dgamma = the chunks' sums in chunk order ------------------------------------------------
__global__ __launch_bounds__(BA_THREADS) void tnet_bnact_param_grads_kernel(const float* __restrict__ part, int n_chunks, int C,
                                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * BA_THREADS + threadIdx.x;
    if (c >= C) return;
    float t1 = 0.f, t2 = 0.f;
    for (int t = 0; t < n_chunks; ++t) {
        t1 += part[((int64_t)t * 2) * C + c];
        t2 += part[((int64_t)t * 2 + 1) * C + c];
    }
    dbeta[c] = t1;
    dgamma[c] = t2;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_desc(const ghn3_bnact_desc* g, bool frozen) {
    if (!g) { ghn3_set_error("bn_act: null descriptor"); return GHN3_E_ARG; }
    if (g->P <= 0 || g->C <= 0) { ghn3_set_error("bn_act: non-positive size in the descriptor"); return GHN3_E_ARG; }
    if (g->relu != 0 && g->relu != 1) { ghn3_set_error("bn_act: relu %d is neither 0 nor 1", g->relu); return GHN3_E_ARG; }
    if (g->C % 4) { ghn3_set_error("bn_act: C %d must be a multiple of 4", g->C); return GHN3_E_LIMIT; }
    if (g->C > BA_MAX_C) { ghn3_set_error("bn_act: C %d is above %d", g->C, BA_MAX_C); return GHN3_E_LIMIT; }
    if ((int64_t)g->P * g->C >= BA_MAX_ELEMS) { ghn3_set_error("bn_act: tensors of 2^31 elements or more are not supported"); return GHN3_E_LIMIT; }
    if (!frozen && g->P < 2) { ghn3_set_error("bn_act: batch statistics need at least 2 values per channel"); return GHN3_E_LIMIT; }
    return GHN3_OK;
}

int check_ptrs(const char* what, std::initializer_list<const void*> quads, std::initializer_list<const void*> others) {
    for (const void* p : quads) {
        if (!p) { ghn3_set_error("%s: null pointer", what); return GHN3_E_ARG; }
        if (!aligned16(p)) { ghn3_set_error("%s: an activation tensor must start on 16 bytes", what); return GHN3_E_ARG; }
    }
    for (const void* p : others)
        if (!p) { ghn3_set_error("%s: null pointer", what); return GHN3_E_ARG; }
    return GHN3_OK;
}

}  // namespace

extern "C" int64_t ghn3_bn_act_scratch_floats(const ghn3_bnact_desc* desc, int mode) {
    if (mode < 0 || mode > 3) { ghn3_set_error("bn_act: mode %d is not backward | 2 frozen", mode); return GHN3_E_ARG; }
    const int rc = check_desc(desc, (mode & 2) != 0);
    if (rc) return rc;
    if (mode == 2) return 0;                                                   // (the frozen forward is one launch)
    return al((int64_t)2 * plan_of(desc->P, desc->C).n_chunks * desc->C);
}

extern "C" int ghn3_bn_act_fwd(const ghn3_bnact_desc* desc, const float* x, const float* gamma, const float* beta, float* out,
                               float* stats, float* scratch, void* stream) {
    int rc = check_desc(desc, false);
    if (rc || (rc = check_ptrs("bn_act fwd", {x, out}, {gamma, beta, stats, scratch}))) return rc;
    const ghn3_bnact_desc& d = *desc;
    const Plan pl = plan_of(d.P, d.C);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tnet_bnact_stats_partial_kernel, dim3(pl.n_chunks, pl.gy), dim3(BA_THREADS), 0, s, x, scratch, d.P, d.C, pl.rows_chunk);
    TNET_LAUNCH_CHECK("bn_act fwd (partial statistics)")
    hipLaunchKernelGGL(tnet_bnact_apply_kernel<false>, dim3(pl.n_rb, pl.gy), dim3(BA_THREADS), 0, s, x, (const float*)scratch, gamma, beta,
                       (const float*)nullptr, (const float*)nullptr, out, stats, d.P, d.C, d.relu, d.eps, pl.rows_chunk, pl.n_chunks,
                       pl.rows_rb);
    TNET_LAUNCH_CHECK("bn_act fwd (apply)")
    return GHN3_OK;
}

extern "C" int ghn3_bn_act_bwd(const ghn3_bnact_desc* desc, const float* dout, const float* x, const float* stats, const float* gamma,
                               const float* beta, float* dx, float* dgamma, float* dbeta, float* scratch, void* stream) {
    int rc = check_desc(desc, false);
    if (rc || (rc = check_ptrs("bn_act bwd", {dout, x, dx}, {stats, gamma, beta, dgamma, dbeta, scratch}))) return rc;
    const ghn3_bnact_desc& d = *desc;
    const Plan pl = plan_of(d.P, d.C);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tnet_bnact_bwd_partial_kernel<false>, dim3(pl.n_chunks, pl.gy), dim3(BA_THREADS), 0, s, dout, x, stats,
                       (const float*)nullptr, (const float*)nullptr, gamma, beta, scratch, (float*)nullptr, d.P, d.C, d.relu, d.eps,
                       pl.rows_chunk);
    TNET_LAUNCH_CHECK("bn_act bwd (partial sums)")
    hipLaunchKernelGGL(tnet_bnact_dx_kernel, dim3(pl.n_rb, pl.gy), dim3(BA_THREADS), 0, s, dout, x, stats, gamma, beta,
                       (const float*)scratch, dx, dgamma, dbeta, d.P, d.C, d.relu, pl.n_chunks, pl.rows_rb);
    TNET_LAUNCH_CHECK("bn_act bwd (dx)")
    return GHN3_OK;
}

extern "C" int ghn3_bn_act_frozen_fwd(const ghn3_bnact_desc* desc, const float* x, const float* gamma, const float* beta,
                                      const float* mean, const float* var, float* out, void* stream) {
    int rc = check_desc(desc, true);
    if (rc || (rc = check_ptrs("bn_act frozen fwd", {x, out}, {gamma, beta, mean, var}))) return rc;
    const ghn3_bnact_desc& d = *desc;
    const Plan pl = plan_of(d.P, d.C);
    hipLaunchKernelGGL(tnet_bnact_apply_kernel<true>, dim3(pl.n_rb, pl.gy), dim3(BA_THREADS), 0, (hipStream_t)stream, x,
                       (const float*)nullptr, gamma, beta, mean, var, out, (float*)nullptr, d.P, d.C, d.relu, d.eps, pl.rows_chunk,
                       pl.n_chunks, pl.rows_rb);
    TNET_LAUNCH_CHECK("bn_act frozen fwd")
    return GHN3_OK;
}

extern "C" int ghn3_bn_act_frozen_bwd(const ghn3_bnact_desc* desc, const float* dout, const float* x, const float* gamma,
                                      const float* beta, const float* mean, const float* var, float* dx, float* dgamma, float* dbeta,
                                      float* scratch, void* stream) {
    int rc = check_desc(desc, true);
    if (rc || (rc = check_ptrs("bn_act frozen bwd", {dout, x, dx}, {gamma, beta, mean, var, dgamma, dbeta, scratch}))) return rc;
    const ghn3_bnact_desc& d = *desc;
    const Plan pl = plan_of(d.P, d.C);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tnet_bnact_bwd_partial_kernel<true>, dim3(pl.n_chunks, pl.gy), dim3(BA_THREADS), 0, s, dout, x,
                       (const float*)nullptr, mean, var, gamma, beta, scratch, dx, d.P, d.C, d.relu, d.eps, pl.rows_chunk);
    TNET_LAUNCH_CHECK("bn_act frozen bwd (dx and partial sums)")
    hipLaunchKernelGGL(tnet_bnact_param_grads_kernel, dim3((d.C + BA_THREADS - 1) / BA_THREADS), dim3(BA_THREADS), 0, s,
                       (const float*)scratch, pl.n_chunks, d.C, dgamma, dbeta);
    TNET_LAUNCH_CHECK("bn_act frozen bwd (parameter gradients)")
    return GHN3_OK;
}
