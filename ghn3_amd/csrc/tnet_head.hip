// Target-network end: the classifier head (global average pool or flatten, then Linear [-> ReLU -> Dropout -> Linear]*,
// ghn3/ops.py:565-569, built at ops.py:489-494) forward and backward, and the label-smoothed cross-entropy with the top-1 / top-5
// hit counts over every network of a meta-batch (trainer.py:195-212).
//
//     f      = mean_hw x   (glob_avg)   or   x flattened in logical NCHW order (c, h, w)          x NCHW or NHWC storage
//     h_1    = f W_1^T + b_1
//     a_j    = relu(h_j) m_j / (1 - p_j)                   (m_j: the uint8 dropout keep mask; none: m = 1, p = 0)
//     h_j+1  = a_j W_j+1^T + b_j+1,    logits = h_n        [B][K]
//
//   forward   head_feat       f [B][F] row-major (skipped for a flattened NCHW x: x itself is f);
//             head_fwd_lin    one launch per linear: a workgroup owns a 16-column tile and 16 RT rows, its four waves take
//                             interleaved k steps and sum their tiles in LDS in wave order; the epilogue adds the bias and,
//                             between linears, applies ReLU, the mask and the scale.  The a_j are kept for the backward.
//   backward  head_dgrad      one launch per linear, last first: dA = G_j W_j; between linears G_j-1 = dA (a_j-1 > 0 ? s : 0),
//                             for the first linear dx (the pooling's broadcast / the flatten's scatter) in x's layout;
//             tnet_wgrad      (tnet_wgrad.hip) every dW_j = G_j^T a_j-1 and db_j = column sums of G_j in one launch: 256-row
//                             chunks, each 32 x 32 output block a workgroup; with one chunk (B <= 256) written in place,
//             tnet_reduce     (tnet_wgrad.hip) else as fixed-order partials summed here.
//   xent      xent_fwd        a workgroup per network (up to 32 networks per launch, their pointers in the kernel arguments),
//                             a wave per row: ce[n], the row log-sum-exps for the backward, the integer hit counts;
//             xent_bwd        a wave per (network, row): dlogits = g_n / B (softmax - (1 - eps) onehot - eps / K).
//
// Every product runs on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate; the stock head is fp32 under autocast
// too).  Instruction j of a 16-wide k step takes k = k0 + 4 (lane >> 4) + j for both operands, a permutation of the summation
// order only.  No float atomics: reruns are bit-identical (the hit counts are integer adds).  Limits (host-checked, mirrored by
// target_ops.ClassifierHead.applicable): 1 <= n_lin <= 4, B <= 4096, F <= 32768, hidden and output widths <= 4096, K >= 1,
// element counts < 2^31.

#include <math.h>
#include "tnet_common.h"

namespace {

constexpr int NT = 256;                     // threads per workgroup (4 waves)
constexpr int MAXL = GHN3_HEAD_MAX_LINEAR;
static_assert(MAXL <= TNET_WG_MAX && MAXL <= TNET_RED_MAX, "one tnet_wgrad / tnet_reduce launch takes every linear");
constexpr int MAX_B = 4096, MAX_F = 32768, MAX_D = 4096;

// Y[rows][Nout] tile (rows r0 .. r0 + 16 RT, columns 16 ct .. 16 ct + 16) = A op(W):
//   A [rows][lda] row-major (K columns read);  WT = false: W [Nout][K] (nn.Linear, Y = A W^T);  WT = true: W [K][Nout], Y = A W.
// The four waves take the k steps k0 = 16 (wave + 4 t); their tiles meet in `red` (4 RT 256 floats of LDS) and are summed in
// wave order.  epi(row, col, value) once per element inside [rows) x [Nout), consecutive threads on consecutive columns.
template <int RT, bool WT, class Epi>
__device__ inline void tile_gemm(const float* __restrict__ A, int lda, int rows, const float* __restrict__ W, int K, int Nout,
                                 int r0, int ct, float* red, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int n = ct * 16 + i;
    const bool nok = n < Nout;
    f32x4 acc[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = wave * 16; k0 < K; k0 += 64) {
        float b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * q + j;
            b[j] = (nok && k < K) ? (WT ? W[(size_t)k * Nout + n] : W[(size_t)n * K + k]) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int ra = r0 + r * 16 + i;
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * q + j;
                a[j] = (ra < rows && k < K) ? A[(size_t)ra * lda + k] : 0.f;
            }
            acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc[r], 0, 0, 0);
            acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc[r], 0, 0, 0);
            acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc[r], 0, 0, 0);
            acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc[r], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) *reinterpret_cast<f32x4*>(red + ((wave * RT + r) * 64 + lane) * 4) = acc[r];
    __syncthreads();
    // C/D of lane l, register g: row 4 (l >> 4) + g, column l & 15
    for (int e = threadIdx.x; e < RT * 256; e += NT) {
        const int r = e >> 8, rr = (e >> 4) & 15, cc = e & 15, l = (rr >> 2) * 16 + cc, g = rr & 3;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) v += red[((w * RT + r) * 64 + l) * 4 + g];
        const int row = r0 + r * 16 + rr, col = ct * 16 + cc;
        if (row < rows && col < Nout) epi(row, col, v);
    }
}

// ------------------------------------------------------------------------------------------------ forward
struct FeatArgs { const float* x; float* f; int B, C, HW, layout, glob_avg; };

__global__ __launch_bounds__(NT) void head_feat_kernel(FeatArgs a) {
    const int F = a.glob_avg ? a.C : a.C * a.HW;
    if (a.glob_avg && a.layout == 0) {                       // NCHW mean: a wave per (b, c) row of HW floats
        const int lane = threadIdx.x & 63, row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
        if (row >= a.B * a.C) return;
        const float* p = a.x + (size_t)row * a.HW;
        float s = 0.f;
        for (int t = lane; t < a.HW; t += 64) s += p[t];
        s = wave_sum(s);
        if (lane == 0) a.f[row] = s / (float)a.HW;
        return;
    }
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= a.B * F) return;
    const int b = e / F, j = e - b * F;
    if (a.glob_avg) {                                        // NHWC mean: a thread per (b, c), consecutive threads on c
        const float* p = a.x + (size_t)b * a.HW * a.C + j;
        float s = 0.f;
        for (int t = 0; t < a.HW; ++t) s += p[(size_t)t * a.C];
        a.f[e] = s / (float)a.HW;
    } else {                                                 // NHWC flatten in (c, h, w) order
        const int c = j / a.HW, hw = j - c * a.HW;
        a.f[e] = a.x[((size_t)b * a.HW + hw) * a.C + c];
    }
}

struct FwdLin {
    const float* A; const float* W; const float* bias; float* Y;
    const unsigned char* mask;               // [rows][Nout] or null
    float scale;
    int rows, K, Nout, act;                  // act: ReLU (+ mask, scale) in the epilogue
};

template <int RT>
__global__ __launch_bounds__(NT) void head_fwd_lin_kernel(FwdLin a) {
    __shared__ float red[4 * RT * 256];
    tile_gemm<RT, false>(a.A, a.K, a.rows, a.W, a.K, a.Nout, blockIdx.y * 16 * RT, blockIdx.x, red, [&](int r, int n, float v) {
        v += a.bias[n];
        const size_t o = (size_t)r * a.Nout + n;
        if (a.act) {
            v = fmaxf(v, 0.f);
            if (a.mask) v = a.mask[o] ? v * a.scale : 0.f;
        }
        a.Y[o] = v;
    });
}

// ------------------------------------------------------------------------------------------------ backward
struct BwdLin {
    const float* G; const float* W; float* Y;
    const float* act;                        // a_j-1 [rows][Nout] (mode 0)
    float scale;
    int rows, K, Nout, mode;                 // mode 0: Y = dA (act > 0 ? scale : 0); mode 1: dx
    int C, HW, layout, glob_avg;             // (mode 1)
};

template <int RT>
__global__ __launch_bounds__(NT) void head_dgrad_kernel(BwdLin a) {
    __shared__ float red[4 * RT * 256];
    tile_gemm<RT, true>(a.G, a.K, a.rows, a.W, a.K, a.Nout, blockIdx.y * 16 * RT, blockIdx.x, red, [&](int r, int n, float v) {
        if (a.mode == 0) {
            const size_t o = (size_t)r * a.Nout + n;
            a.Y[o] = a.act[o] > 0.f ? v * a.scale : 0.f;
        } else if (a.glob_avg) {                 // mean backward: dx[b, c, :, :] = df[b][c] / HW
            const float g = v / (float)a.HW;
            if (a.layout) {
                float* p = a.Y + (size_t)r * a.HW * a.C + n;
                for (int t = 0; t < a.HW; ++t) p[(size_t)t * a.C] = g;
            } else {
                float* p = a.Y + ((size_t)r * a.C + n) * a.HW;
                for (int t = 0; t < a.HW; ++t) p[t] = g;
            }
        } else if (a.layout) {                   // flatten backward, NHWC: feature (c, hw) -> [b][hw][c]
            const int c = n / a.HW, hw = n - c * a.HW;
            a.Y[((size_t)r * a.HW + hw) * a.C + c] = v;
        } else {
            a.Y[(size_t)r * a.Nout + n] = v;
        }
    });
}

// ------------------------------------------------------------------------------------------------ cross-entropy
struct XentTable { const float* p[GHN3_XENT_MAX_NETS]; };
struct XentArgs { const int64_t* targets; float* ce; float* lse; int* hits; int B, K, n0; float eps; };

// a workgroup per network, a wave per row: row losses into LDS, then their mean in row order
__global__ __launch_bounds__(1024) void xent_fwd_kernel(XentTable logits, XentArgs a) {
    __shared__ float row_loss[MAX_B];
    __shared__ int hit_cnt[2][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const float* L = logits.p[blockIdx.x];
    const int net = a.n0 + blockIdx.x;
    int h1 = 0, h5 = 0;
    for (int r = wave; r < a.B; r += nw) {
        const float* z = L + (size_t)r * a.K;
        const int64_t t = a.targets[r];
        const bool valid = t >= 0 && t < a.K;
        float m = -INFINITY;
        for (int k = lane; k < a.K; k += 64) m = fmaxf(m, z[k]);
        m = wave_max(m);
        const float zt = valid ? z[t] : 0.f;
        float se = 0.f, sz = 0.f;
        int gt = 0;
        for (int k = lane; k < a.K; k += 64) {
            const float v = z[k];
            se += expf(v - m);
            sz += v;
            gt += v > zt;
        }
        se = wave_sum(se);
        sz = wave_sum(sz);
        gt = wave_isum(gt);
        const float lse = m + logf(se);
        if (lane == 0) {
            float loss = NAN;
            if (valid) {
                loss = (1.f - a.eps) * (lse - zt);
                if (a.eps != 0.f) loss += a.eps * (lse - sz / (float)a.K);
            }
            row_loss[r] = loss;
            a.lse[(size_t)net * a.B + r] = lse;
            h1 += valid && gt < 1;
            h5 += valid && gt < 5;
        }
    }
    if (lane == 0) { hit_cnt[0][wave] = h1; hit_cnt[1][wave] = h5; }
    __syncthreads();
    if (wave == 0) {
        float s = 0.f;
        for (int r = lane; r < a.B; r += 64) s += row_loss[r];
        s = wave_sum(s);
        if (lane == 0) {
            a.ce[net] = s / (float)a.B;
            int c1 = 0, c5 = 0;
            for (int w = 0; w < nw; ++w) { c1 += hit_cnt[0][w]; c5 += hit_cnt[1][w]; }
            atomicAdd(a.hits, c1);                              // (integer adds: exact in any order)
            atomicAdd(a.hits + 1, c5);
        }
    }
}

struct XentBwdTable { const float* p[GHN3_XENT_MAX_NETS]; float* d[GHN3_XENT_MAX_NETS]; };
struct XentBwdArgs { const int64_t* targets; const float* lse; const float* dce; int B, K, n0; float eps; };

// grid (networks, row groups of 4): a wave per row
__global__ __launch_bounds__(NT) void xent_bwd_kernel(XentBwdTable tab, XentBwdArgs a) {
    const int lane = threadIdx.x & 63, r = blockIdx.y * (NT / 64) + (threadIdx.x >> 6);
    if (r >= a.B) return;
    const int net = a.n0 + blockIdx.x;
    const float* z = tab.p[blockIdx.x] + (size_t)r * a.K;
    float* dz = tab.d[blockIdx.x] + (size_t)r * a.K;
    const int64_t t = a.targets[r];
    const bool valid = t >= 0 && t < a.K;
    const float lse = a.lse[(size_t)net * a.B + r];
    const float g = a.dce[net] / (float)a.B, off = a.eps / (float)a.K;
    for (int k = lane; k < a.K; k += 64) {
        const float p = expf(z[k] - lse);
        dz[k] = valid ? g * (p - (k == t ? 1.f - a.eps : 0.f) - off) : NAN;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct HeadDims {
    int B, C, H, W, HW, layout, glob_avg, n, direct;
    int d[MAXL + 1];
    float scale[MAXL - 1];
};

int check(const ghn3_head_desc* g, HeadDims* out) {
    if (!g) { ghn3_set_error("head: null descriptor"); return GHN3_E_ARG; }
    const ghn3_head_desc& s = *g;
    if (s.B <= 0 || s.C <= 0 || s.H <= 0 || s.W <= 0) { ghn3_set_error("head: non-positive size in the descriptor"); return GHN3_E_ARG; }
    if (s.layout != 0 && s.layout != 1) { ghn3_set_error("head: layout %d is neither 0 (NCHW) nor 1 (NHWC)", s.layout); return GHN3_E_ARG; }
    if (s.glob_avg != 0 && s.glob_avg != 1) { ghn3_set_error("head: glob_avg %d is neither 0 nor 1", s.glob_avg); return GHN3_E_ARG; }
    if (s.n_lin < 1 || s.n_lin > MAXL) { ghn3_set_error("head: %d linear layers (1 .. %d)", s.n_lin, MAXL); return GHN3_E_LIMIT; }
    const int64_t HW = (int64_t)s.H * s.W, F = s.glob_avg ? (int64_t)s.C : s.C * HW;
    if (s.dims[0] != F) {
        ghn3_set_error("head: dims[0] = %d is not the feature size %lld", s.dims[0], (long long)F);
        return GHN3_E_ARG;
    }
    for (int j = 1; j <= s.n_lin; ++j)
        if (s.dims[j] <= 0) { ghn3_set_error("head: dims[%d] = %d", j, s.dims[j]); return GHN3_E_ARG; }
    for (int j = 0; j + 1 < s.n_lin; ++j)
        if (!(s.p[j] >= 0.f && s.p[j] < 1.f)) { ghn3_set_error("head: dropout rate %g outside [0, 1)", (double)s.p[j]); return GHN3_E_ARG; }
    if (s.B > MAX_B) { ghn3_set_error("head: batch %d (limit %d)", s.B, MAX_B); return GHN3_E_LIMIT; }
    if (F > MAX_F) { ghn3_set_error("head: %lld features (limit %d)", (long long)F, MAX_F); return GHN3_E_LIMIT; }
    for (int j = 1; j <= s.n_lin; ++j)
        if (s.dims[j] > MAX_D) { ghn3_set_error("head: width %d of linear %d (limit %d)", s.dims[j], j, MAX_D); return GHN3_E_LIMIT; }
    if ((int64_t)s.B * s.C * HW >= (1ll << 31)) { ghn3_set_error("head: tensors of 2^31 elements or more are not supported"); return GHN3_E_LIMIT; }
    if (out) {
        HeadDims d{};
        d.B = s.B; d.C = s.C; d.H = s.H; d.W = s.W; d.HW = (int)HW; d.layout = s.layout; d.glob_avg = s.glob_avg; d.n = s.n_lin;
        d.direct = !s.glob_avg && s.layout == 0;
        for (int j = 0; j <= s.n_lin; ++j) d.d[j] = s.dims[j];
        for (int j = 0; j + 1 < s.n_lin; ++j) d.scale[j] = 1.f / (1.f - s.p[j]);
        *out = d;
    }
    return GHN3_OK;
}

// forward scratch (kept for the backward): f (absent when x is f) | a_1 .. a_n-1
struct FwdLayout { int64_t f, a[MAXL], total; };
FwdLayout fwd_layout(const HeadDims& d) {
    FwdLayout L{};
    int64_t o = 0;
    L.f = o; if (!d.direct) o += al((int64_t)d.B * d.d[0]);
    for (int j = 1; j < d.n; ++j) { L.a[j] = o; o += al((int64_t)d.B * d.d[j]); }
    L.total = o;
    return L;
}

// backward scratch: G_1 .. G_n-1 | partials of every linear (more than one row chunk only)
struct BwdLayout { int64_t g[MAXL], part[MAXL + 1], total; };
BwdLayout bwd_layout(const HeadDims& d) {
    BwdLayout L{};
    int64_t o = 0;
    for (int j = 1; j < d.n; ++j) { L.g[j] = o; o += al((int64_t)d.B * d.d[j]); }
    for (int j = 1; j <= d.n; ++j) {
        L.part[j] = o;
        if (tnet_wg_chunks(d.B) > 1) o += tnet_wg_part_floats(d.B, d.d[j], d.d[j - 1]);
    }
    L.total = o;
    return L;
}

// 64-row blocks where that still gives 128 workgroups, else 16-row ones
bool wide_rows(int rows, int Nout) { return rows >= 64 && (int64_t)((rows + 63) / 64) * ((Nout + 15) / 16) >= 128; }

int launch_fwd_lin(const FwdLin& a, hipStream_t s) {
    const int tiles = (a.Nout + 15) / 16;
    if (wide_rows(a.rows, a.Nout))
        hipLaunchKernelGGL(head_fwd_lin_kernel<4>, dim3(tiles, (a.rows + 63) / 64), dim3(NT), 0, s, a);
    else
        hipLaunchKernelGGL(head_fwd_lin_kernel<1>, dim3(tiles, (a.rows + 15) / 16), dim3(NT), 0, s, a);
    TNET_LAUNCH_CHECK("head linear");
    return GHN3_OK;
}

int launch_dgrad(const BwdLin& a, hipStream_t s) {
    const int tiles = (a.Nout + 15) / 16;
    if (wide_rows(a.rows, a.Nout))
        hipLaunchKernelGGL(head_dgrad_kernel<4>, dim3(tiles, (a.rows + 63) / 64), dim3(NT), 0, s, a);
    else
        hipLaunchKernelGGL(head_dgrad_kernel<1>, dim3(tiles, (a.rows + 15) / 16), dim3(NT), 0, s, a);
    TNET_LAUNCH_CHECK("head dgrad");
    return GHN3_OK;
}

}  // namespace

extern "C" int64_t ghn3_head_scratch_floats(const ghn3_head_desc* desc, int backward) {
    HeadDims d;
    const int rc = check(desc, &d);
    if (rc) return rc;
    return backward ? bwd_layout(d).total : fwd_layout(d).total;
}

extern "C" int ghn3_head_fwd(const ghn3_head_desc* desc, const float* x, const ghn3_head_params* params, float* logits,
                             float* scratch, void* stream) {
    HeadDims d;
    int rc = check(desc, &d);
    if (rc) return rc;
    if (!x || !logits || !params || (!scratch && fwd_layout(d).total > 0)) { ghn3_set_error("head fwd: null pointer"); return GHN3_E_ARG; }
    for (int j = 0; j < d.n; ++j)
        if (!params->w[j] || !params->b[j]) { ghn3_set_error("head fwd: null weight or bias of linear %d", j + 1); return GHN3_E_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const FwdLayout L = fwd_layout(d);
    const float* f = x;
    if (!d.direct) {
        FeatArgs fa{x, scratch + L.f, d.B, d.C, d.HW, d.layout, d.glob_avg};
        const int blocks = d.glob_avg && !d.layout ? (d.B * d.C + NT / 64 - 1) / (NT / 64) : (d.B * d.d[0] + NT - 1) / NT;
        hipLaunchKernelGGL(head_feat_kernel, dim3(blocks), dim3(NT), 0, s, fa);
        TNET_LAUNCH_CHECK("head feat");
        f = scratch + L.f;
    }
    for (int j = 1; j <= d.n; ++j) {
        const bool last = j == d.n;
        const unsigned char* m = last ? nullptr : params->mask[j - 1];
        FwdLin a{j == 1 ? f : scratch + L.a[j - 1], params->w[j - 1], params->b[j - 1], last ? logits : scratch + L.a[j], m,
                 (last || !m) ? 1.f : d.scale[j - 1], d.B, d.d[j - 1], d.d[j], !last};
        if ((rc = launch_fwd_lin(a, s))) return rc;
    }
    return GHN3_OK;
}

extern "C" int ghn3_head_bwd(const ghn3_head_desc* desc, const float* dlogits, const float* x, const ghn3_head_params* params,
                             const float* fwd_scratch, float* dx, const ghn3_head_grads* grads, float* scratch, void* stream) {
    HeadDims d;
    int rc = check(desc, &d);
    if (rc) return rc;
    const FwdLayout F = fwd_layout(d);
    const BwdLayout L = bwd_layout(d);
    if (!dlogits || !x || !params || !dx || !grads || (!fwd_scratch && F.total > 0) || (!scratch && L.total > 0)) {
        ghn3_set_error("head bwd: null pointer");
        return GHN3_E_ARG;
    }
    for (int j = 0; j < d.n; ++j)
        if (!params->w[j] || !grads->w[j] || !grads->b[j]) { ghn3_set_error("head bwd: null weight or gradient of linear %d", j + 1); return GHN3_E_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const float* fwd_a[MAXL + 1];                // X operand of linear j: a_j-1 (f for j = 1)
    fwd_a[1] = d.direct ? x : fwd_scratch + F.f;
    for (int j = 2; j <= d.n; ++j) fwd_a[j] = fwd_scratch + F.a[j - 1];
    const float* G[MAXL + 1];                    // gradient at the output of linear j
    G[d.n] = dlogits;
    for (int j = 1; j < d.n; ++j) G[j] = scratch + L.g[j];
    for (int j = d.n; j >= 1; --j) {
        BwdLin a{};
        a.G = G[j]; a.W = params->w[j - 1]; a.rows = d.B; a.K = d.d[j]; a.Nout = d.d[j - 1];
        if (j > 1) {
            a.mode = 0; a.Y = scratch + L.g[j - 1]; a.act = fwd_a[j];
            a.scale = params->mask[j - 2] ? d.scale[j - 2] : 1.f;
        } else {
            a.mode = 1; a.Y = dx; a.C = d.C; a.HW = d.HW; a.layout = d.layout; a.glob_avg = d.glob_avg;
        }
        if ((rc = launch_dgrad(a, s))) return rc;
    }
    // every dW_j = G_j^T a_j-1 and db_j in one launch: in place with one row chunk, else partials and their sums
    const bool parts = tnet_wg_chunks(d.B) > 1;
    TnetWgProb wg[MAXL];
    TnetRedProb red[MAXL];
    for (int j = 1; j <= d.n; ++j) {
        wg[j - 1] = TnetWgProb{G[j], fwd_a[j], parts ? scratch + L.part[j] : nullptr, grads->w[j - 1], grads->b[j - 1],
                               d.B, d.d[j], d.d[j - 1], 1};
        red[j - 1] = tnet_wg_reduce(wg[j - 1]);
    }
    if ((rc = tnet_wgrad_launch(wg, d.n, s))) return rc;
    if (parts && (rc = tnet_reduce_launch(red, d.n, s))) return rc;
    return GHN3_OK;
}

namespace {
int xent_check(const ghn3_xent_desc* g) {
    if (!g) { ghn3_set_error("xent: null descriptor"); return GHN3_E_ARG; }
    if (g->n_nets <= 0 || g->B <= 0 || g->K <= 0) { ghn3_set_error("xent: non-positive size in the descriptor"); return GHN3_E_ARG; }
    if (g->B > MAX_B) { ghn3_set_error("xent: batch %d (limit %d)", g->B, MAX_B); return GHN3_E_LIMIT; }
    if ((int64_t)g->B * g->K >= (1ll << 31)) { ghn3_set_error("xent: logits of 2^31 elements or more are not supported"); return GHN3_E_LIMIT; }
    return GHN3_OK;
}
}  // namespace

extern "C" int ghn3_xent_fwd(const ghn3_xent_desc* desc, const float* const* logits, const int64_t* targets, float* ce, float* lse,
                             int32_t* hits, void* stream) {
    int rc = xent_check(desc);
    if (rc) return rc;
    if (!logits || !targets || !ce || !lse || !hits) { ghn3_set_error("xent fwd: null pointer"); return GHN3_E_ARG; }
    const ghn3_xent_desc& g = *desc;
    hipStream_t s = (hipStream_t)stream;
    for (int n0 = 0; n0 < g.n_nets; n0 += GHN3_XENT_MAX_NETS) {
        const int cnt = g.n_nets - n0 < GHN3_XENT_MAX_NETS ? g.n_nets - n0 : GHN3_XENT_MAX_NETS;
        XentTable t{};
        for (int i = 0; i < cnt; ++i) {
            if (!logits[n0 + i]) { ghn3_set_error("xent fwd: null logits of network %d", n0 + i); return GHN3_E_ARG; }
            t.p[i] = logits[n0 + i];
        }
        const int threads = g.B >= 1024 ? 1024 : ((g.B + 63) / 64) * 64;
        hipLaunchKernelGGL(xent_fwd_kernel, dim3(cnt), dim3(threads), 0, s, t,
                           XentArgs{targets, ce, lse, (int*)hits, g.B, g.K, n0, g.eps});
        TNET_LAUNCH_CHECK("xent fwd");
    }
    return GHN3_OK;
}

extern "C" int ghn3_xent_bwd(const ghn3_xent_desc* desc, const float* const* logits, const int64_t* targets, const float* lse,
                             const float* dce, float* const* dlogits, void* stream) {
    int rc = xent_check(desc);
    if (rc) return rc;
    if (!logits || !targets || !lse || !dce || !dlogits) { ghn3_set_error("xent bwd: null pointer"); return GHN3_E_ARG; }
    const ghn3_xent_desc& g = *desc;
    hipStream_t s = (hipStream_t)stream;
    for (int n0 = 0; n0 < g.n_nets; n0 += GHN3_XENT_MAX_NETS) {
        const int cnt = g.n_nets - n0 < GHN3_XENT_MAX_NETS ? g.n_nets - n0 : GHN3_XENT_MAX_NETS;
        XentBwdTable t{};
        for (int i = 0; i < cnt; ++i) {
            if (!logits[n0 + i] || !dlogits[n0 + i]) { ghn3_set_error("xent bwd: null pointer of network %d", n0 + i); return GHN3_E_ARG; }
            t.p[i] = logits[n0 + i];
            t.d[i] = dlogits[n0 + i];
        }
        hipLaunchKernelGGL(xent_bwd_kernel, dim3(cnt, (g.B + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, s, t,
                           XentBwdArgs{targets, lse, dce, g.B, g.K, n0, g.eps});
        TNET_LAUNCH_CHECK("xent bwd");
    }
    return GHN3_OK;
}
