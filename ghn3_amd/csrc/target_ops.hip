// Target-network execution, first native slice: the dominant chain of the DeepNets-1M search space,
//
//     ReLU -> depthwise k x k convolution (stride, dilation) -> pointwise 1 x 1 convolution -> BatchNorm (batch statistics)
//
// = `DilConv` and each half of `SepConv` (/root/reference/ghn3/ops.py:198-240), forward and backward, as one op family on
// NHWC (channels-last) fp32 activations.  The reference runs it as four ATen / MIOpen modules per direction (ReLU, grouped
// conv, 1x1 conv, batch norm: ~9 passes over the activations forward, more backward) with weights the GHN predicted; here
//
//   forward   dwpw_fwd      one pass: ReLU + depthwise taps produce a [64 pixels x 32 channels] operand chunk in LDS, the
//                           pointwise product runs on the bf16 matrix cores with SPLIT operands: both factors as three bf16
//                           pieces (24 bits of mantissa) and six products -- fp32's own rounding, ~1e-7; the matrix work is
//                           free here, the op is memory- and launch-bound -- fp32 accumulate, against weight chunks converted
//                           while staged (two pieces, ~1e-5, for more than 256 output columns per workgroup: registers), the epilogue writes the pre-norm activations z once and leaves per-tile
//                           (mean, M2) of every channel;
//             bn_finalize   Chan-combines the tiles in a fixed order -> mean, rstd;   bn_apply  normalises (one pass).
//   backward  bn_bwd_partial + reduce_rows   sum dout, sum dout.xhat -> dgamma, dbeta;
//             dwpw_bwd_data  dz is formed on the fly from (dout, z, statistics) as the operand of dy = dz W_pw (matrix
//                            cores, same split arithmetic);
//             pw_wgrad       dW_pw = dz^T y over pixel chunks: dz formed on the fly again, y RE-COMPUTED from x (never
//                            stored), partial products per chunk + fixed-order reduction;
//             dw_bwd_data    dx = 1[x > 0] . transposed depthwise taps of dy;   dw_wgrad  dW_dw partials + reduction.
//
// Everything is HBM-bound (K = C_in <= 512: a few hundred flops per byte at most), so the design minimises passes: x is read
// by three kernels, z by three, nothing else of activation size except dy is materialised.  All reductions are deterministic
// (fixed-order partial slots).  Weights are read IN PLACE: w_dw [C_in][ks][ks], w_pw [C_out][C_in], gamma / beta [C_out] are
// views of the GHN's flat prediction buffer; their gradients are written densely for autograd to route back into it.
// Limits (checked by the host): C_in, C_out multiples of 4 and <= 512, ks <= 7 (odd or even), N H W C < 2^31.
// WIDE networks (the `wide` evaluation split of DeepNets-1M: up to 2048 channels in the last stage, 8192 into a cell's 1 x 1
// preprocessing layer): a chain with max(C_in, C_out) > 512 runs as two nodes -- the depthwise stage alone (ghn3_dw_fwd / _bwd:
// tnet_dw_fwd_kernel, C <= 16384) and the pointwise convolution + norm on the dense-convolution family, which takes C_out <= 4096,
// C_in <= 16384 (its kernels split the columns over the grid and walk the reduction in chunks; tnet_bn_bwd_partial_kernel loops
// over the channel quads above 1024 channels).  Squeeze-and-excitation takes C, J <= 4096 (se_pixel_sum loops above 1024).  At or
// below the former widths (512 / 1024) every kernel takes the code path, launch geometry and summation order it had.
// w_dw == nullptr (ks = 1): the same family as ReLU -> 1x1 convolution (stride) -> BatchNorm = `ReLUConvBN` with a 1x1 kernel,
// the preprocessing layer of every cell and the `conv_1x1` op (ops.py:180-198): the depthwise stage degenerates to the ReLU.
// Without a norm layer (ghn3_dwpw_plain_fwd / _bwd: the blocks of a network built with norm = None, ops.py:91-96, whose norm slots
// are Identity layers): the same kernels with NORM = false.  The forward is dwpw_fwd alone -- its accumulators are the output, no
// z, no statistics --; in the backward dz IS dout, so dwpw_bwd_data and pw_wgrad load it plainly and bn_bwd_partial is not run:
// one launch forward, six backward, nothing of activation size kept between them but x.
// With a norm layer that normalises with RUNNING statistics (ghn3_dwpw_frozen_fwd / _bwd, ghn3_conv_frozen_fwd / _bwd: a
// BatchNorm in eval mode): the same kernels with NORM = NORM_FROZEN.  The norm is a per-channel affine map whose constants are
// known before the launch, so the forward applies it to its accumulators in the epilogue -- no statistics, no second pass --
// and the backward has dz = dout gamma rstd without the two batch-mean terms; dgamma / dbeta come from bn_bwd_partial +
// reduce_rows on the frozen (mean, rstd).
// With the ReLU BEHIND the norm layer and an optional skip tensor in between (ghn3_conv_bn_act_*, ghn3_conv_frozen_act_*: the
// layer order of ResNet-shaped torch.nn networks): sibling kernels of bn_apply, bn_bwd_partial and the dz pass (tnet_bn_act_apply,
// tnet_bn_act_bwd_partial, tnet_dz_act) around the unchanged convolution, weight-gradient and reduction kernels.

#include <algorithm>
#include "tnet_common.h"

namespace {

constexpr int TP = 64;       // pixels per tile (4 waves x 16-row MFMA tiles)
// (KC, LDK and the split-bf16 product helpers splitS / frag / mma_terms: tnet_common.h, shared with tnet_patch.hip)
constexpr int MAXT = 49;     // taps (ks <= 7)
// operand pieces of the kernels templated on NT (16 NT columns per workgroup): three (fp32-equivalent products) up to 256
// columns, two for the widest tiles (registers)
constexpr int terms_of(int NT) { return NT <= 16 ? 3 : 2; }

struct Desc {
    int N, H, W, C_in, C_out, ks, stride, pad, dil, Ho, Wo;
    float eps;
};

// What follows the convolution (the NORM template parameter of the kernels): nothing, a BatchNorm with batch statistics, or a
// BatchNorm with frozen (running) statistics.
constexpr int NORM_NONE = 0, NORM_BATCH = 1, NORM_FROZEN = 2;

// The constants of a BatchNorm with frozen statistics, [C_out] each, and where the forward stores its result (NORM_FROZEN
// only; a zero-filled struct otherwise).
struct Frozen {
    const float *gamma, *beta, *mean, *var;
    float* out;
};

// (v - mean) rstd gamma + beta of the four consecutive channels col .. col + 3 a lane owns in a fragment: four-float loads of
// the constants, rstd = 1 / sqrt(var + eps) as tnet_bn_finalize_kernel forms it, the expression of tnet_bn_apply_kernel
__device__ __forceinline__ f32x4 frozen_affine4(const f32x4 v, const Frozen& fz, int col, float eps) {
    const f32x4 mu = *reinterpret_cast<const f32x4*>(fz.mean + col), va = *reinterpret_cast<const f32x4*>(fz.var + col);
    const f32x4 ga = *reinterpret_cast<const f32x4*>(fz.gamma + col), be = *reinterpret_cast<const f32x4*>(fz.beta + col);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (v[e] - mu[e]) * (1.f / sqrtf(va[e] + eps)) * ga[e] + be[e];
    return o;
}

// ReLU + depthwise taps of 8 consecutive channels c .. c + 7 at output pixel (n, oh, ow); ih0 / iw0 = input origin of the
// pixel's window; wt = taps x `wld` floats in LDS, channel cc of the chunk at wt[t * wld + cc]
__device__ __forceinline__ void dw_taps8(const float* __restrict__ x, const Desc& d, int n, int ih0, int iw0, int c,
                                         const float* wt, int wld, int cc, float (&out)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = 0.f;
    if (n < 0 || c >= d.C_in) return;
    const bool second = c + 4 < d.C_in;
    int t = 0;
    for (int kh = 0; kh < d.ks; ++kh) {
        const int ih = ih0 + kh * d.dil;
        for (int kw = 0; kw < d.ks; ++kw, ++t) {
            const int iw = iw0 + kw * d.dil;
            if (ih < 0 || ih >= d.H || iw < 0 || iw >= d.W) continue;
            const float* px = x + ((int64_t)(n * d.H + ih) * d.W + iw) * d.C_in + c;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(px);
            const f32x4 v1 = second ? *reinterpret_cast<const f32x4*>(px + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            const float* w = wt + t * wld + cc;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                out[e] = fmaf(fmaxf(v0[e], 0.f), w[e], out[e]);
                out[4 + e] = fmaf(fmaxf(v1[e], 0.f), w[4 + e], out[4 + e]);
            }
        }
    }
}

__device__ __forceinline__ void decode_pixel(const Desc& d, int p, int P, int& n, int& ih0, int& iw0) {
    if (p >= P) { n = -1; ih0 = iw0 = 0; return; }
    const int hw = d.Ho * d.Wo;
    n = p / hw;
    const int r = p - n * hw, oh = r / d.Wo, ow = r - oh * d.Wo;
    ih0 = oh * d.stride - d.pad;
    iw0 = ow * d.stride - d.pad;
}

// dz of 8 consecutive channels of output pixel p:  gamma rstd (dout - s1 / P - xhat s2 / P),  xhat = (z - mean) rstd
__device__ __forceinline__ void dz8(const float* __restrict__ dout, const float* __restrict__ z, const float* __restrict__ stats,
                                    const float* __restrict__ gamma, const float* __restrict__ s12, int C, int p, int P, int c,
                                    float (&out)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = 0.f;
    if (p >= P) return;
    const float invP = 1.f / (float)P;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int cc = c + 4 * h;
        if (cc >= C) break;
        const f32x4 g = *reinterpret_cast<const f32x4*>(dout + (int64_t)p * C + cc);
        const f32x4 zz = *reinterpret_cast<const f32x4*>(z + (int64_t)p * C + cc);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(stats + cc), rs = *reinterpret_cast<const f32x4*>(stats + C + cc);
        const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + cc);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(s12 + cc), a2 = *reinterpret_cast<const f32x4*>(s12 + C + cc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (zz[e] - mu[e]) * rs[e];
            out[4 * h + e] = ga[e] * rs[e] * (g[e] - a1[e] * invP - xh * a2[e] * invP);
        }
    }
}

// 8 consecutive channels c .. c + 7 of row p of dz [P][C]; zeros for p >= P and for channels at or beyond C
__device__ __forceinline__ void dz_in8(const float* __restrict__ dz, int C, int p, int P, int c, float (&out)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = 0.f;
    if (p >= P) return;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int cc = c + 4 * h;
        if (cc >= C) break;
        const f32x4 g = *reinterpret_cast<const f32x4*>(dz + (int64_t)p * C + cc);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[4 * h + e] = g[e];
    }
}

// dz of 8 consecutive channels behind a norm layer with frozen statistics: gamma rstd dout (stats = mean | rstd)
__device__ __forceinline__ void dz_frozen8(const float* __restrict__ dout, const float* __restrict__ stats,
                                           const float* __restrict__ gamma, int C, int p, int P, int c, float (&out)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = 0.f;
    if (p >= P) return;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int cc = c + 4 * h;
        if (cc >= C) break;
        const f32x4 g = *reinterpret_cast<const f32x4*>(dout + (int64_t)p * C + cc);
        const f32x4 rs = *reinterpret_cast<const f32x4*>(stats + C + cc), ga = *reinterpret_cast<const f32x4*>(gamma + cc);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[4 * h + e] = ga[e] * rs[e] * g[e];
    }
}

// The operand rows of the backward products: NORM_BATCH forms dz from (dout, z, statistics); NORM_NONE -- the family without a
// norm layer -- has dz = dout, a plain load (z, stats, gamma, s12 are not touched); NORM_FROZEN scales dout by gamma rstd (z and
// s12 are not touched).
template <int NORM>
__device__ __forceinline__ void dz_operand8(const float* __restrict__ dout, const float* __restrict__ z, const float* __restrict__ stats,
                                            const float* __restrict__ gamma, const float* __restrict__ s12, int C, int p, int P, int c,
                                            float (&out)[8]) {
    if constexpr (NORM == NORM_BATCH) dz8(dout, z, stats, gamma, s12, C, p, P, c, out);
    else if constexpr (NORM == NORM_FROZEN) dz_frozen8(dout, stats, gamma, C, p, P, c, out);
    else dz_in8(dout, C, p, P, c, out);
}

// ---------------------------------------------------------------------------------------------------------------------
// forward: z = pw(dw(relu(x))), per-tile channel statistics.  NORM_NONE: z is the op's output and the kernel ends with its
// store (no statistics, `part` not touched, no `red` section in LDS).  NORM_FROZEN: the affine map of the frozen norm layer is
// applied to the accumulators and stored to fz.out; z (the pre-affine result the backward reads) is stored as well when it is
// non-null; no statistics, `part` and `red` as for NORM_NONE.
// ---------------------------------------------------------------------------------------------------------------------
template <int NT, int NORM = NORM_BATCH>
__global__ __launch_bounds__(256) void tnet_dwpw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w_dw,
                                                            const float* __restrict__ w_pw, float* __restrict__ z,
                                                            float* __restrict__ part, const Desc d, const int P, const Frozen fz) {
    constexpr int S = terms_of(NT);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* pix = reinterpret_cast<int*>(smem);                                   // [3][TP]
    float* wt = reinterpret_cast<float*>(smem + 3 * TP * 4);                   // [MAXT][KC]
    unsigned short* As = reinterpret_cast<unsigned short*>(smem + 3 * TP * 4 + MAXT * KC * 4);      // [S][TP][LDK]
    unsigned short* Bs = As + S * TP * LDK;                                                          // [S][16 NT][LDK]
    [[maybe_unused]] float* red = reinterpret_cast<float*>(Bs + S * 16 * NT * LDK);   // [5][16 NT] (NORM_BATCH only)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, kc = lane >> 4;
    const int tile = blockIdx.x, p0 = tile * TP, taps = d.ks * d.ks;
    if (tid < TP) {
        int n, ih0, iw0;
        decode_pixel(d, p0 + tid, P, n, ih0, iw0);
        pix[tid] = n; pix[TP + tid] = ih0; pix[2 * TP + tid] = iw0;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < d.C_in; c0 += KC) {
        __syncthreads();                                                       // (previous chunk's fragments are consumed)
        for (int i = tid; i < taps * KC; i += 256) {
            const int t = i / KC, cc = i % KC, c = c0 + cc;
            wt[t * KC + cc] = c < d.C_in ? (w_dw ? w_dw[(int64_t)c * taps + t] : 1.f) : 0.f;
        }
        for (int i = tid; i < 16 * NT * 8; i += 256) {
            const int n = i >> 3, k = (i & 7) * 4, c = c0 + k;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (n < d.C_out && c < d.C_in) v = *reinterpret_cast<const f32x4*>(w_pw + (int64_t)n * d.C_in + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) splitS<S>(v[e], Bs, n * LDK + k + e, 16 * NT * LDK);
        }
        __syncthreads();
        {
            const int i = tid >> 2, cc = (tid & 3) * 8;
            float y[8];
            dw_taps8(x, d, pix[i], pix[TP + i], pix[2 * TP + i], c0 + cc, wt, KC, cc, y);
#pragma unroll
            for (int e = 0; e < 8; ++e) splitS<S>(y[e], As, i * LDK + cc + e, TP * LDK);
        }
        __syncthreads();
        u16x8 af[S];
#pragma unroll
        for (int q = 0; q < S; ++q) af[q] = frag(As + q * TP * LDK, 16 * w + r16, kc);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (16 * j < d.C_out) {
                u16x8 bf[S];
#pragma unroll
                for (int q = 0; q < S; ++q) bf[q] = frag(Bs + q * 16 * NT * LDK, 16 * j + r16, kc);
                acc[j] = mma_terms<S>(af, bf, acc[j]);
            }
        }
    }
    // ---- epilogue: z, then per-tile (mean, M2) of every channel
    const int prow = p0 + 16 * w + r16;
    const bool valid = prow < P;
    if constexpr (NORM == NORM_FROZEN) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = 16 * j + 4 * kc;
            if (valid && col < d.C_out) {
                if (z) *reinterpret_cast<f32x4*>(z + (int64_t)prow * d.C_out + col) = acc[j];
                *reinterpret_cast<f32x4*>(fz.out + (int64_t)prow * d.C_out + col) = frozen_affine4(acc[j], fz, col, d.eps);
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = 16 * j + 4 * kc;
        if (valid && col < d.C_out) *reinterpret_cast<f32x4*>(z + (int64_t)prow * d.C_out + col) = acc[j];
    }
    if constexpr (NORM == NORM_BATCH) {
        const int cnt = min(TP, P - p0);
        auto tile_sum = [&](bool centred) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = 16 * j + 4 * kc;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = 0.f;
                    if (valid) { v = acc[j][e]; if (centred) { v -= red[4 * 16 * NT + col + e]; v *= v; } }
                    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
                    if (r16 == 0) red[w * 16 * NT + col + e] = v;
                }
            }
            __syncthreads();
        };
        tile_sum(false);
        for (int c = tid; c < 16 * NT; c += 256)
            red[4 * 16 * NT + c] = (red[c] + red[16 * NT + c] + red[2 * 16 * NT + c] + red[3 * 16 * NT + c]) / (float)cnt;
        tile_sum(true);
        for (int c = tid; c < d.C_out; c += 256) {
            part[((int64_t)tile * 2) * d.C_out + c] = red[4 * 16 * NT + c];
            part[((int64_t)tile * 2 + 1) * d.C_out + c] = red[c] + red[16 * NT + c] + red[2 * 16 * NT + c] + red[3 * 16 * NT + c];
        }
    }
}

// (mean, M2) of the tiles -> stats[0..C) = mean, stats[C..2C) = 1 / sqrt(var + eps), stats[2C..3C) = biased variance.
// 16 channels per workgroup x 16 tile lanes; lane g combines tiles g, g + 16, ... in order, then the 16 lanes in order.
__global__ __launch_bounds__(256) void tnet_bn_finalize_kernel(const float* __restrict__ part, int n_tiles, int P, int C, float eps,
                                                               float* __restrict__ stats) {
    __shared__ float sn[16][16], sm[16][16], s2[16][16];
    const int cl = threadIdx.x & 15, g = threadIdx.x >> 4, c = blockIdx.x * 16 + cl;
    float n = 0.f, mean = 0.f, M2 = 0.f;
    if (c < C)
        for (int t = g; t < n_tiles; t += 16) {
            const float nb = (float)min(TP, P - t * TP), mb = part[((int64_t)t * 2) * C + c], Mb = part[((int64_t)t * 2 + 1) * C + c];
            const float nn = n + nb, dl = mb - mean;
            mean += dl * nb / nn;
            M2 += Mb + dl * dl * n * nb / nn;
            n = nn;
        }
    sn[g][cl] = n; sm[g][cl] = mean; s2[g][cl] = M2;
    __syncthreads();
    if (g == 0 && c < C) {
        for (int q = 1; q < 16; ++q) {
            const float nb = sn[q][cl];
            if (nb > 0.f) {
                const float nn = n + nb, dl = sm[q][cl] - mean;
                mean += dl * nb / nn;
                M2 += s2[q][cl] + dl * dl * n * nb / nn;
                n = nn;
            }
        }
        const float var = M2 / n;
        stats[c] = mean;
        stats[C + c] = 1.f / sqrtf(var + eps);
        stats[2 * C + c] = var;
    }
}

__global__ __launch_bounds__(256) void tnet_bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ stats,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ out, int64_t total4, int C) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % C);
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + i * 4);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(stats + c), rs = *reinterpret_cast<const f32x4*>(stats + C + c);
        const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c), be = *reinterpret_cast<const f32x4*>(beta + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (v[e] - mu[e]) * rs[e] * ga[e] + be[e];
        *reinterpret_cast<f32x4*>(out + i * 4) = o;
    }
}

// The "act" member of the dense-convolution family (conv -> BatchNorm [-> + skip] -> ReLU, the layer order of ResNet-shaped
// networks): tnet_bn_apply_kernel with the skip tensor `res` [P][C] (null: none) added behind the affine map -- torch's order: norm,
// add, clamp -- and the result clamped at zero as torch's ReLU does (a NaN stays one).  Nothing of activation size is read
// beyond z and res.
constexpr int ACT_GRID_CAP = 2048;                                             // workgroups of the two flat kernels of the member
__global__ __launch_bounds__(256) void tnet_bn_act_apply_kernel(const float* __restrict__ z, const float* __restrict__ stats,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ res, float* __restrict__ out,
                                                                int64_t total4, int C) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % C);
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + i * 4);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(stats + c), rs = *reinterpret_cast<const f32x4*>(stats + C + c);
        const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c), be = *reinterpret_cast<const f32x4*>(beta + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (v[e] - mu[e]) * rs[e] * ga[e] + be[e];
        if (res) {
            const f32x4 r = *reinterpret_cast<const f32x4*>(res + i * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += r[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = o[e] <= 0.f ? 0.f : o[e];
        *reinterpret_cast<f32x4*>(out + i * 4) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------
// per 64-pixel tile: part[tile][0][c] = sum dout, part[tile][1][c] = sum dout xhat.  Up to 256 channel quads (C <= 1024) the
// threads are (quad) x (pixel group) and the groups are added through LDS; wider layers (launched without LDS) give every thread
// the quads tid, tid + 256, ... over the tile's pixels in sequence and write the sums directly.
__global__ __launch_bounds__(256) void tnet_bn_bwd_partial_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                                  const float* __restrict__ stats, float* __restrict__ part,
                                                                  int P, int C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);                               // [ng][2][C]
    const int nq = C / 4, ng = max(1, 256 / nq);
    const int g = threadIdx.x / nq, q = threadIdx.x % nq, c = 4 * q;
    const int p0 = blockIdx.x * TP, p1 = min(P, p0 + TP);
    if (nq > 256) {
        for (int cw = 4 * threadIdx.x; cw < C; cw += 1024) {
            f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
            const f32x4 mu = *reinterpret_cast<const f32x4*>(stats + cw), rs = *reinterpret_cast<const f32x4*>(stats + C + cw);
            for (int p = p0; p < p1; ++p) {
                const f32x4 gd = *reinterpret_cast<const f32x4*>(dout + (int64_t)p * C + cw);
                const f32x4 zz = *reinterpret_cast<const f32x4*>(z + (int64_t)p * C + cw);
#pragma unroll
                for (int e = 0; e < 4; ++e) { s1[e] += gd[e]; s2[e] += gd[e] * (zz[e] - mu[e]) * rs[e]; }
            }
            *reinterpret_cast<f32x4*>(part + (int64_t)blockIdx.x * 2 * C + cw) = s1;
            *reinterpret_cast<f32x4*>(part + (int64_t)blockIdx.x * 2 * C + C + cw) = s2;
        }
        return;
    }
    if (g < ng) {
        f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
        const f32x4 mu = *reinterpret_cast<const f32x4*>(stats + c), rs = *reinterpret_cast<const f32x4*>(stats + C + c);
        for (int p = p0 + g; p < p1; p += ng) {
            const f32x4 gd = *reinterpret_cast<const f32x4*>(dout + (int64_t)p * C + c);
            const f32x4 zz = *reinterpret_cast<const f32x4*>(z + (int64_t)p * C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s1[e] += gd[e]; s2[e] += gd[e] * (zz[e] - mu[e]) * rs[e]; }
        }
        *reinterpret_cast<f32x4*>(red + (g * 2) * C + c) = s1;
        *reinterpret_cast<f32x4*>(red + (g * 2 + 1) * C + c) = s2;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        float s = 0.f;
        for (int k = 0; k < ng; ++k) s += red[k * 2 * C + i];
        part[(int64_t)blockIdx.x * 2 * C + i] = s;
    }
}

// The same sums behind the ReLU of the "act" member: the upstream gradient is g = dout 1[out > 0], masked where it is read (torch
// masks on the ReLU's RESULT); `out` [P][C] is the forward's result.  Geometry, LDS and summation order of the kernel above, in
// both of its arms.
__device__ __forceinline__ f32x4 act_masked(const f32x4 g, const f32x4 o) {
    f32x4 m;
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = o[e] > 0.f ? g[e] : 0.f;
    return m;
}
__global__ __launch_bounds__(256) void tnet_bn_act_bwd_partial_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                                      const float* __restrict__ z, const float* __restrict__ stats,
                                                                      float* __restrict__ part, int P, int C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);                               // [ng][2][C]
    const int nq = C / 4, ng = max(1, 256 / nq);
    const int g = threadIdx.x / nq, q = threadIdx.x % nq, c = 4 * q;
    const int p0 = blockIdx.x * TP, p1 = min(P, p0 + TP);
    if (nq > 256) {
        for (int cw = 4 * threadIdx.x; cw < C; cw += 1024) {
            f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
            const f32x4 mu = *reinterpret_cast<const f32x4*>(stats + cw), rs = *reinterpret_cast<const f32x4*>(stats + C + cw);
            for (int p = p0; p < p1; ++p) {
                const f32x4 gd = act_masked(*reinterpret_cast<const f32x4*>(dout + (int64_t)p * C + cw),
                                            *reinterpret_cast<const f32x4*>(out + (int64_t)p * C + cw));
                const f32x4 zz = *reinterpret_cast<const f32x4*>(z + (int64_t)p * C + cw);
#pragma unroll
                for (int e = 0; e < 4; ++e) { s1[e] += gd[e]; s2[e] += gd[e] * (zz[e] - mu[e]) * rs[e]; }
            }
            *reinterpret_cast<f32x4*>(part + (int64_t)blockIdx.x * 2 * C + cw) = s1;
            *reinterpret_cast<f32x4*>(part + (int64_t)blockIdx.x * 2 * C + C + cw) = s2;
        }
        return;
    }
    if (g < ng) {
        f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
        const f32x4 mu = *reinterpret_cast<const f32x4*>(stats + c), rs = *reinterpret_cast<const f32x4*>(stats + C + c);
        for (int p = p0 + g; p < p1; p += ng) {
            const f32x4 gd = act_masked(*reinterpret_cast<const f32x4*>(dout + (int64_t)p * C + c),
                                        *reinterpret_cast<const f32x4*>(out + (int64_t)p * C + c));
            const f32x4 zz = *reinterpret_cast<const f32x4*>(z + (int64_t)p * C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s1[e] += gd[e]; s2[e] += gd[e] * (zz[e] - mu[e]) * rs[e]; }
        }
        *reinterpret_cast<f32x4*>(red + (g * 2) * C + c) = s1;
        *reinterpret_cast<f32x4*>(red + (g * 2 + 1) * C + c) = s2;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        float s = 0.f;
        for (int k = 0; k < ng; ++k) s += red[k * 2 * C + i];
        part[(int64_t)blockIdx.x * 2 * C + i] = s;
    }
}

// out[map(col)] = sum_r part[r][col] in a fixed order; 64 columns per workgroup x 16 row lanes.  tr_c > 0: the columns are
// (t, c) pairs, col = t * tr_c + c, written transposed to out[c * tr_t + t].
__global__ __launch_bounds__(256) void tnet_reduce_rows_kernel(const float* __restrict__ part, int n_rows, int64_t n_cols,
                                                               float* __restrict__ out, int tr_c, int tr_t) {
    __shared__ f32x4 sm[16][16];
    const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int64_t col = ((int64_t)blockIdx.x * 16 + cl) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (col < n_cols)
        for (int r = g; r < n_rows; r += 16) s += *reinterpret_cast<const f32x4*>(part + (int64_t)r * n_cols + col);
    sm[g][cl] = s;
    __syncthreads();
    if (g == 0 && col < n_cols) {
        for (int q = 1; q < 16; ++q) s += sm[q][cl];
        if (tr_c > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t cc = col + e;
                out[(cc % tr_c) * tr_t + cc / tr_c] = s[e];
            }
        } else {
            *reinterpret_cast<f32x4*>(out + col) = s;
        }
    }
}

// dy [P][C_in] = dz [P][C_out] W_pw [C_out][C_in]; dz formed on the fly (dz_operand8)
template <int NT, int NORM = NORM_BATCH>
__global__ __launch_bounds__(256) void tnet_dwpw_bwd_data_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                                 const float* __restrict__ stats, const float* __restrict__ gamma,
                                                                 const float* __restrict__ s12, const float* __restrict__ w_pw,
                                                                 float* __restrict__ dy, const Desc d, const int P) {
    constexpr int S = terms_of(NT);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned short* As = reinterpret_cast<unsigned short*>(smem);              // [S][TP][LDK]
    unsigned short* Bs = As + S * TP * LDK;                                    // [S][16 NT][LDK]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, kc = lane >> 4;
    const int p0 = blockIdx.x * TP;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < d.C_out; c0 += KC) {
        __syncthreads();
        {   // A[i][k] = dz[p0 + i][c0 + k]
            const int i = tid >> 2, cc = (tid & 3) * 8;
            float v[8];
            dz_operand8<NORM>(dout, z, stats, gamma, s12, d.C_out, p0 + i, P, c0 + cc, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) splitS<S>(v[e], As, i * LDK + cc + e, TP * LDK);
        }
        // B[n = ci][k] = W_pw[c0 + k][n]
        for (int i = tid; i < KC * 4 * NT; i += 256) {
            const int k = i / (4 * NT), n = (i % (4 * NT)) * 4, co = c0 + k;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (co < d.C_out && n < d.C_in) v = *reinterpret_cast<const f32x4*>(w_pw + (int64_t)co * d.C_in + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) splitS<S>(v[e], Bs, (n + e) * LDK + k, 16 * NT * LDK);
        }
        __syncthreads();
        u16x8 af[S];
#pragma unroll
        for (int q = 0; q < S; ++q) af[q] = frag(As + q * TP * LDK, 16 * w + r16, kc);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (16 * j < d.C_in) {
                u16x8 bf[S];
#pragma unroll
                for (int q = 0; q < S; ++q) bf[q] = frag(Bs + q * 16 * NT * LDK, 16 * j + r16, kc);
                acc[j] = mma_terms<S>(af, bf, acc[j]);
            }
        }
    }
    const int prow = p0 + 16 * w + r16;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = 16 * j + 4 * kc;
        if (prow < P && col < d.C_in) *reinterpret_cast<f32x4*>(dy + (int64_t)prow * d.C_in + col) = acc[j];
    }
}

// part[chunk][co][ci] = sum over the chunk's pixels of dz[p][co] y[p][ci]; workgroup = (chunk, 64 co, 64 ci)
template <int NORM = NORM_BATCH>
__global__ __launch_bounds__(256) void tnet_pw_wgrad_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                            const float* __restrict__ stats, const float* __restrict__ gamma,
                                                            const float* __restrict__ s12, const float* __restrict__ x,
                                                            const float* __restrict__ w_dw, float* __restrict__ part,
                                                            const Desc d, const int P, const int chunk_px) {
    constexpr int S = 3;
    __shared__ __attribute__((aligned(16))) unsigned short As[S * 64 * LDK], Bs[S * 64 * LDK];
    __shared__ float wt[MAXT * 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, kc = lane >> 4;
    const int chunk = blockIdx.x, co0 = blockIdx.y * 64, ci0 = blockIdx.z * 64, taps = d.ks * d.ks;
    const int pa = chunk * chunk_px, pb = min(P, pa + chunk_px);
    for (int i = tid; i < taps * 64; i += 256) {
        const int t = i >> 6, cc = i & 63, c = ci0 + cc;
        wt[t * 64 + cc] = c < d.C_in ? (w_dw ? w_dw[(int64_t)c * taps + t] : 1.f) : 0.f;
    }
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int pk = pa; pk < pb; pk += KC) {
        __syncthreads();
        const int k = tid >> 3, m8 = (tid & 7) * 8, p = pk + k;
        {   // A[m = co][k = pixel]
            float v[8];
            dz_operand8<NORM>(dout, z, stats, gamma, s12, d.C_out, p < pb ? p : P, P, co0 + m8, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) splitS<S>(v[e], As, (m8 + e) * LDK + k, 64 * LDK);
        }
        {   // B[n = ci][k = pixel] = y re-computed
            int n, ih0, iw0;
            decode_pixel(d, p < pb ? p : P, P, n, ih0, iw0);
            float y[8];
            dw_taps8(x, d, n, ih0, iw0, ci0 + m8, wt, 64, m8, y);
#pragma unroll
            for (int e = 0; e < 8; ++e) splitS<S>(y[e], Bs, (m8 + e) * LDK + k, 64 * LDK);
        }
        __syncthreads();
        u16x8 af[S];
#pragma unroll
        for (int q = 0; q < S; ++q) af[q] = frag(As + q * 64 * LDK, 16 * w + r16, kc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u16x8 bf[S];
#pragma unroll
            for (int q = 0; q < S; ++q) bf[q] = frag(Bs + q * 64 * LDK, 16 * j + r16, kc);
            acc[j] = mma_terms<S>(af, bf, acc[j]);
        }
    }
    const int co = co0 + 16 * w + r16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = ci0 + 16 * j + 4 * kc;
        if (co < d.C_out && ci < d.C_in)
            *reinterpret_cast<f32x4*>(part + ((int64_t)chunk * d.C_out + co) * d.C_in + ci) = acc[j];
    }
}

// dx[n, ih, iw, c] = 1[x > 0] sum over the taps that read this input: dy[n, oh, ow, c] w_dw[c][kh][kw]
__global__ __launch_bounds__(256) void tnet_dw_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               const float* __restrict__ w_dw, float* __restrict__ dx,
                                                               const Desc d, int64_t total4) {
    const int nq = d.C_in / 4, taps = d.ks * d.ks;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % nq) * 4;
        int64_t pix = i / nq;
        const int iw = (int)(pix % d.W);
        pix /= d.W;
        const int ih = (int)(pix % d.H), n = (int)(pix / d.H);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kh = 0; kh < d.ks; ++kh) {
            const int th = ih + d.pad - kh * d.dil;
            if (th < 0 || th % d.stride) continue;
            const int oh = th / d.stride;
            if (oh >= d.Ho) continue;
            for (int kw = 0; kw < d.ks; ++kw) {
                const int tw = iw + d.pad - kw * d.dil;
                if (tw < 0 || tw % d.stride) continue;
                const int ow = tw / d.stride;
                if (ow >= d.Wo) continue;
                const f32x4 g = *reinterpret_cast<const f32x4*>(dy + ((int64_t)(n * d.Ho + oh) * d.Wo + ow) * d.C_in + c);
                const int t = kh * d.ks + kw;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(g[e], w_dw ? w_dw[(int64_t)(c + e) * taps + t] : 1.f, acc[e]);
            }
        }
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = xv[e] > 0.f ? acc[e] : 0.f;
        *reinterpret_cast<f32x4*>(dx + i * 4) = acc;
    }
}

// part[chunk][t][c] = sum over the chunk's output pixels of dy[p][c] relu(x[tap t of p][c])
__global__ __launch_bounds__(256) void tnet_dw_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            float* __restrict__ part, const Desc d, const int P, const int chunk_px) {
    // Threads = (channel quad) x (pixel lane): a thread sums its channels over every PL-th pixel of the chunk for up to TG taps at
    // a time (registers), the pixel lanes are then added through LDS.  (One (tap, channel quad) per
    // thread, walking the chunk's 128 pixels in sequence, keeps taps x C / 4 of the 256 threads busy: 108 us per call, 9 ms of
    // the training loop's 75 ms of GPU time per step.)  More than 256 channel quads (the stand-alone depthwise op of wide
    // networks): slices of 256 quads on blockIdx.y, each of them the same scheme; one slice = the grid and the sums as before.
    constexpr int TG = 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f32x4* red = reinterpret_cast<f32x4*>(smem);                               // [PL][TG][nq]
    const int q0 = blockIdx.y * 256, nq = min(256, d.C_in / 4 - q0), taps = d.ks * d.ks, PL = max(1, 256 / nq);
    const int cq = threadIdx.x % nq, pl = threadIdx.x / nq;
    const bool live = pl < PL;
    dy += 4 * q0; x += 4 * q0; part += 4 * q0;                                 // (this slice's first channel)
    const int pa = blockIdx.x * chunk_px, pb = min(P, pa + chunk_px);
    const int hw = d.Ho * d.Wo;
    for (int t0 = 0; t0 < taps; t0 += TG) {
        f32x4 acc[TG];
#pragma unroll
        for (int tt = 0; tt < TG; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (live) {
            for (int p = pa + pl; p < pb; p += PL) {
                const int n = p / hw, r = p - n * hw, oh = r / d.Wo, ow = r - oh * d.Wo;
                const int ih0 = oh * d.stride - d.pad, iw0 = ow * d.stride - d.pad;
                const f32x4 g = *reinterpret_cast<const f32x4*>(dy + (int64_t)p * d.C_in + 4 * cq);
                const float* xn = x + (int64_t)n * d.H * d.W * d.C_in + 4 * cq;
#pragma unroll
                for (int tt = 0; tt < TG; ++tt) {
                    const int t = t0 + tt;
                    if (t < taps) {
                        const int kh = t / d.ks, kw = t - kh * d.ks;
                        const int ih = ih0 + kh * d.dil, iw = iw0 + kw * d.dil;
                        if (ih >= 0 && ih < d.H && iw >= 0 && iw < d.W) {
                            const f32x4 xv = *reinterpret_cast<const f32x4*>(xn + ((int64_t)ih * d.W + iw) * d.C_in);
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[tt][e] = fmaf(g[e], fmaxf(xv[e], 0.f), acc[tt][e]);
                        }
                    }
                }
            }
        }
        __syncthreads();                                                       // (the previous tap group's sums have been read)
        if (live) {
#pragma unroll
            for (int tt = 0; tt < TG; ++tt) red[(pl * TG + tt) * nq + cq] = acc[tt];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < TG * nq; i += 256) {
            const int tt = i / nq, c4 = i - tt * nq, t = t0 + tt;
            if (t >= taps) continue;
            f32x4 sum = red[tt * nq + c4];
            for (int l = 1; l < PL; ++l) {
                const f32x4 v = red[(l * TG + tt) * nq + c4];
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[e] += v[e];
            }
            *reinterpret_cast<f32x4*>(part + ((int64_t)blockIdx.x * taps + t) * d.C_in + 4 * c4) = sum;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The DENSE convolution chain  [ReLU ->] kh x kw convolution (stride, padding, dilation) -> BatchNorm
// = `ReLUConvBN` with a k x k kernel (the `conv_3x3 / 5x5 / 7x7` ops, /root/reference/ghn3/ops.py:180-198, 297) and its
// 1 x k / k x 1 halves.  Implicit GEMM on the same machinery as the depthwise / pointwise family above: a workgroup owns 64
// output pixels x a group of output channels, the reduction runs over (tap, 32 input channels) chunks -- the operand chunk of a
// tap is the (ReLU of the) shifted input pixels, read straight from x; the weights come as bf16 pieces from a
// [piece][tap][C_out][C_in] pack of the predicted [C_out][C_in][kh][kw] tensor (one small launch) -- split operands with three
// bf16 pieces, fp32 accumulate, z + per-tile statistics in the epilogue.  Backward: dz written once (tnet_dz_kernel); dx by the
// transposed implicit GEMM over the taps that read an input pixel (the same kernel, on the transposed pack); dW per (tap,
// 64 x 64 block, pixel chunk) partials + fixed-order reduction, written back in the parameter's own [C_out][C_in][kh][kw]
// order.  The stock path runs these layers as MIOpen implicit-GEMM / Winograd kernels between two layout transposes, ~4
// launches forward and ~8 backward per layer, plus ReLU and BatchNorm launches.
// Here: the descriptor and the weight-gradient kernel; tnet_conv_w_pack_kernel, tnet_dz_kernel and tnet_conv2_kernel follow the
// host side of the depthwise / pointwise family.
// ---------------------------------------------------------------------------------------------------------------------
struct CDesc {
    int N, H, W, C_in, C_out, kh, kw, sh, sw, ph, pw, dil, Ho, Wo, relu;
    float eps;
};

// (relu of) 8 consecutive channels c .. c + 7 of input pixel (n, ih, iw); zeros outside the image / beyond C_in
__device__ __forceinline__ void conv_in8(const float* __restrict__ x, const CDesc& d, int n, int ih, int iw, int c, float (&out)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = 0.f;
    if (n < 0 || c >= d.C_in || ih < 0 || ih >= d.H || iw < 0 || iw >= d.W) return;
    const float* px = x + ((int64_t)(n * d.H + ih) * d.W + iw) * d.C_in + c;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(px);
    const f32x4 v1 = c + 4 < d.C_in ? *reinterpret_cast<const f32x4*>(px + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        out[e] = d.relu ? fmaxf(v0[e], 0.f) : v0[e];
        out[4 + e] = d.relu ? fmaxf(v1[e], 0.f) : v1[e];
    }
}

// part[chunk][t][co][ci] = sum over the chunk's output pixels of dz[p][co] act(x[tap t of p][ci]); workgroup = (chunk, 64 co, (t, 64 ci))
__global__ __launch_bounds__(256) void tnet_conv_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                              float* __restrict__ part, const CDesc d, const int P, const int chunk_px) {
    // (the loads of pixel step k + 1 are in flight during the products of step k: registers -> the other LDS stage, one barrier
    // per step)
    constexpr int S = 3;
    constexpr int STAGE = S * 64 * LDK;
    __shared__ __attribute__((aligned(16))) unsigned short As[2 * STAGE], Bs[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, kc = lane >> 4;
    const int ci_tiles = (d.C_in + 63) / 64, taps = d.kh * d.kw;
    const int chunk = blockIdx.x, co0 = blockIdx.y * 64, t = blockIdx.z / ci_tiles, ci0 = (blockIdx.z % ci_tiles) * 64;
    const int dh = (t / d.kw) * d.dil, dw_ = (t % d.kw) * d.dil;
    const int pa = chunk * chunk_px, pb = min(P, pa + chunk_px), hw = d.Ho * d.Wo;
    // Thread = (pixel k of the step, 8 consecutive channels m8 ..): lanes of a wave hold 32 consecutive pixels of two channel
    // groups.  The operands need the pixel index along k, i.e. a transposition on the way into LDS: neighbouring lanes (pixels
    // k, k + 1) exchange halves so that every lane writes 32-bit words (two pixels of one channel) -- 12 conflict-free stores per
    // operand instead of 24 two-byte ones that collided four ways (two-byte stores: 118 us per call).
    const int k = tid & 31, m8 = (tid >> 5) * 8;
    float va[8], vb[8];
    auto put = [&](const float (&v)[8], unsigned short* base) {
        const bool odd = k & 1;
        // even lanes take channels 0..3 of both pixels (k, k + 1), odd lanes channels 4..7: four floats change lanes
        float lo[4], hi[4];                                                    // values at the even / the odd pixel of the pair
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float got = __shfl_xor(odd ? v[e] : v[4 + e], 1, 64);
            lo[e] = odd ? got : v[e];
            hi[e] = odd ? v[4 + e] : got;
        }
        unsigned* row = reinterpret_cast<unsigned*>(base + (m8 + (odd ? 4 : 0)) * LDK + (k & ~1));
#pragma unroll
        for (int q = 0; q < S; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned h = bf16_pk(lo[e], hi[e]);
                row[(q * 64 * LDK + e * LDK) / 2] = h;
                lo[e] -= __uint_as_float(h << 16);
                hi[e] -= __uint_as_float(h & 0xffff0000u);
            }
        }
    };
    auto fetch = [&](int pk) {
        const int p = pk + k;
        dz_in8(dz, d.C_out, p < pb ? p : P, P, co0 + m8, va);                            // A[m = co][k = pixel]
        int n = -1, ih = 0, iw = 0;                                                      // B[n = ci][k = pixel]: act(x) at the tap's input pixel
        if (p < pb) {
            n = p / hw;
            const int r = p - n * hw, oh = r / d.Wo, ow = r - oh * d.Wo;
            ih = oh * d.sh - d.ph + dh; iw = ow * d.sw - d.pw + dw_;
        }
        conv_in8(x, d, n, ih, iw, ci0 + m8, vb);
    };
    auto stage = [&](int buf) {
        put(va, As + buf * STAGE);
        put(vb, Bs + buf * STAGE);
    };
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(pa);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int pk = pa; pk < pb; pk += KC, buf ^= 1) {
        const bool more = pk + KC < pb;
        if (more) fetch(pk + KC);
        u16x8 af[S];
#pragma unroll
        for (int q = 0; q < S; ++q) af[q] = frag(As + buf * STAGE + q * 64 * LDK, 16 * w + r16, kc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u16x8 bf[S];
#pragma unroll
            for (int q = 0; q < S; ++q) bf[q] = frag(Bs + buf * STAGE + q * 64 * LDK, 16 * j + r16, kc);
            acc[j] = mma_terms<S>(af, bf, acc[j]);
        }
        if (more) stage(buf ^ 1);
        __syncthreads();
    }
    const int co = co0 + 16 * w + r16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = ci0 + 16 * j + 4 * kc;
        if (co < d.C_out && ci < d.C_in)
            *reinterpret_cast<f32x4*>(part + (((int64_t)chunk * taps + t) * d.C_out + co) * d.C_in + ci) = acc[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
inline int nt_of(int C) { return C <= 64 ? 4 : C <= 128 ? 8 : C <= 256 ? 16 : 32; }
inline size_t fwd_lds(int NT, bool norm = true) { const int S = terms_of(NT); return 3 * TP * 4 + MAXT * KC * 4 + S * TP * LDK * 2 + S * 16 * NT * LDK * 2 + (norm ? 5 * 16 * NT * 4 : 0); }
inline size_t bwd_lds(int NT) { const int S = terms_of(NT); return S * TP * LDK * 2 + S * 16 * NT * LDK * 2; }

struct Plan { int P, n_tiles, pw_chunks, pw_chunk_px, dw_chunks, dw_chunk_px; };

Plan make_plan(const Desc& d) {
    Plan pl;
    pl.P = d.N * d.Ho * d.Wo;
    pl.n_tiles = (pl.P + TP - 1) / TP;
    const int blocks = ((d.C_out + 63) / 64) * ((d.C_in + 63) / 64);
    int chunks = (768 + blocks - 1) / blocks;
    chunks = std::max(1, std::min(chunks, (pl.P + KC - 1) / KC));
    pl.pw_chunk_px = ((pl.P + chunks - 1) / chunks + KC - 1) / KC * KC;
    pl.pw_chunks = (pl.P + pl.pw_chunk_px - 1) / pl.pw_chunk_px;
    pl.dw_chunk_px = std::max(16, std::min(128, ((pl.P + 255) / 256 + 15) / 16 * 16));   // >= 256 workgroups where the image allows
    pl.dw_chunks = (pl.P + pl.dw_chunk_px - 1) / pl.dw_chunk_px;
    return pl;
}

constexpr int DWPW_MAX_C = 512;     // the fused chain: all output columns of a pixel tile in one workgroup's accumulators
constexpr int DW_MAX_C = 16384;     // the depthwise stage alone

// The descriptor check of the family: `who` begins every message, max_c is the width limit, `alone` (the depthwise stage alone,
// ghn3_dw_*) requires C_out == C_in.  The defaults are the fused chain's.
int check_desc(const ghn3_dwpw_desc* g, Desc& d, const char* who = "dwpw", int max_c = DWPW_MAX_C, bool alone = false) {
    if (!g) { ghn3_set_error("%s: null descriptor", who); return GHN3_E_ARG; }
    d = Desc{g->N, g->H, g->W, g->C_in, g->C_out, g->ks, g->stride, g->pad, g->dil, g->Ho, g->Wo, g->eps};
    if (d.N <= 0 || d.H <= 0 || d.W <= 0 || d.C_in <= 0 || (alone ? d.C_out != d.C_in : d.C_out <= 0) || d.ks <= 0 || d.stride <= 0 ||
        d.dil <= 0 || d.pad < 0) {
        ghn3_set_error("%s: non-positive size in the descriptor%s", who, alone ? ", or C_out != C_in" : "");
        return GHN3_E_ARG;
    }
    if ((d.C_in & 3) || (d.C_out & 3) || d.C_in > max_c || d.C_out > max_c || d.ks > 7) {
        if (alone) ghn3_set_error("%s: needs C a multiple of 4 and <= %d, ks <= 7 (got %d, ks %d)", who, max_c, d.C_in, d.ks);
        else ghn3_set_error("%s: needs C_in, C_out multiples of 4 and <= %d, ks <= 7 (got %d -> %d, ks %d)", who, max_c, d.C_in, d.C_out, d.ks);
        return GHN3_E_LIMIT;
    }
    const int ho = (d.H + 2 * d.pad - d.dil * (d.ks - 1) - 1) / d.stride + 1, wo = (d.W + 2 * d.pad - d.dil * (d.ks - 1) - 1) / d.stride + 1;
    if (ho != d.Ho || wo != d.Wo || ho <= 0 || wo <= 0) {
        ghn3_set_error("%s: output size %d x %d does not match the convolution arithmetic (%d x %d)", who, d.Ho, d.Wo, ho, wo);
        return GHN3_E_ARG;
    }
    if ((int64_t)d.N * d.H * d.W * std::max(d.C_in, d.C_out) >= ((int64_t)1 << 31) ||
        (int64_t)d.N * d.Ho * d.Wo * std::max(d.C_in, d.C_out) >= ((int64_t)1 << 31)) {
        ghn3_set_error("%s: activation tensors of 2^31 elements or more are not supported", who);
        return GHN3_E_LIMIT;
    }
    return GHN3_OK;
}

// ---- launch idioms ---------------------------------------------------------------------------------------------------------------
// hipGetLastError after a launch, reported as "<what>: <HIP's text>" (TNET_LAUNCH_CHECK for a name that is not a literal)
inline int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return GHN3_OK;
    ghn3_set_error("%s: %s", what, hipGetErrorString(e));
    return GHN3_E_HIP;
}

// the grid of a flat grid-stride kernel: one thread per item up to `cap` workgroups
inline dim3 grid1d(int64_t items, int cap) { return dim3((int)std::min<int64_t>((items + 255) / 256, cap)); }

// out = the fixed-order sum of the `rows` partial rows of `cols` floats (a, b: tnet_reduce_rows_kernel's transposition, 0, 0 = none)
int reduce_rows(const float* part, int rows, int64_t cols, float* out, int a, int b, hipStream_t s, const char* what) {
    hipLaunchKernelGGL(tnet_reduce_rows_kernel, dim3((int)((cols / 4 + 15) / 16)), dim3(256), 0, s, part, rows, cols, out, a, b);
    return launched(what);
}

// mean | rstd of the batch from the forward's per-tile (mean, M2), then out = (z - mean) rstd gamma + beta: the two launches
// behind the forward kernel of a member with batch statistics
int bn_apply_launch(const float* part, int n_tiles, int P, int C, float eps, const float* z, const float* gamma, const float* beta,
                    float* stats, float* out, hipStream_t s) {
    hipLaunchKernelGGL(tnet_bn_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, s, part, n_tiles, P, C, eps, stats);
    TNET_LAUNCH_CHECK("bn finalize")
    const int64_t total4 = (int64_t)P * C / 4;
    hipLaunchKernelGGL(tnet_bn_apply_kernel, grid1d(total4, 4096), dim3(256), 0, s, z, stats, gamma, beta, out, total4, C);
    TNET_LAUNCH_CHECK("bn apply")
    return GHN3_OK;
}

// (mean, var) of a frozen norm layer -> stats[0..C) = mean, stats[C..2C) = 1 / sqrt(var + eps): what tnet_bn_bwd_partial_kernel,
// dz_frozen8 and tnet_dz_kernel read
__global__ __launch_bounds__(256) void tnet_bn_frozen_stats_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                                   float eps, int C, float* __restrict__ stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        stats[c] = mean[c];
        stats[C + c] = 1.f / sqrtf(var[c] + eps);
    }
}

// Step 1 of the backward of a norm layer: dbeta = sum dout, dgamma = sum dout xhat over the P pixels (per-tile partials, then a
// fixed-order reduction).  *s12_out = where the reduced pair [sum dout | sum dout xhat] lies: dbeta directly followed by dgamma --
// how target_ops.py lays them out -- IS that pair (no copies); otherwise it is reduced into s12_scratch and copied out.
// act_out != null (the "act" member): the sums of dout 1[act_out > 0], by the sibling kernel in the same launch slot.
int bn_param_grads(const float* dout, const float* z, const float* stats, float* part12, float* s12_scratch, float* dgamma,
                   float* dbeta, int n_tiles, int P, int C, hipStream_t s, const float** s12_out, const float* act_out = nullptr) {
    const bool in_place = dgamma == dbeta + C;
    float* s12 = in_place ? dbeta : s12_scratch;
    const int nq = C / 4, ng = std::max(1, 256 / nq);
    if (act_out) {                                                 // (the "act" member: dout masked by its result, in the same launch)
        hipLaunchKernelGGL(tnet_bn_act_bwd_partial_kernel, dim3(n_tiles), dim3(256), nq > 256 ? 0 : (size_t)ng * 2 * C * 4, s, dout, act_out,
                           z, stats, part12, P, C);
    } else {
        hipLaunchKernelGGL(tnet_bn_bwd_partial_kernel, dim3(n_tiles), dim3(256), nq > 256 ? 0 : (size_t)ng * 2 * C * 4, s, dout, z, stats,
                           part12, P, C);
    }
    TNET_LAUNCH_CHECK("bn bwd partial")
    const int rc = reduce_rows(part12, n_tiles, (int64_t)2 * C, s12, 0, 0, s, "bn bwd reduce");
    if (rc) return rc;
    if (!in_place) {
        (void)hipMemcpyAsync(dbeta, s12, (size_t)C * 4, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(dgamma, s12 + C, (size_t)C * 4, hipMemcpyDeviceToDevice, s);
    }
    *s12_out = s12;
    return GHN3_OK;
}

// dW_dw [C_in][ks][ks] = sum over the output pixels of dy relu(x at the tap): per-chunk partials, then the fixed-order reduction
// that also transposes (tap, channel) to the parameter's order.  LDS = [pixel lanes][16 taps][quads of a slice] float4.
int dw_wgrad(const Desc& d, const Plan& pl, const float* dy, const float* x, float* part_dw, float* dw_dw, hipStream_t s) {
    const int nq = d.C_in / 4, taps = d.ks * d.ks;
    const size_t lds = nq > 256 ? (size_t)65536 : (size_t)std::max(1, 256 / nq) * 16 * nq * 16;
    hipLaunchKernelGGL(tnet_dw_wgrad_kernel, dim3(pl.dw_chunks, (nq + 255) / 256), dim3(256), lds, s, dy, x, part_dw, d, pl.P,
                       pl.dw_chunk_px);
    TNET_LAUNCH_CHECK("dw wgrad")
    return reduce_rows(part_dw, pl.dw_chunks, (int64_t)taps * d.C_in, dw_dw, d.C_in, taps, s, "dw wgrad reduce");
}

// dx = 1[x > 0] . transposed depthwise taps of dy (w_dw == nullptr: the ReLU mask alone)
int dw_bwd_data(const Desc& d, const float* dy, const float* x, const float* w_dw, float* dx, hipStream_t s) {
    const int64_t total4 = (int64_t)d.N * d.H * d.W * d.C_in / 4;
    hipLaunchKernelGGL(tnet_dw_bwd_data_kernel, grid1d(total4, 8192), dim3(256), 0, s, dy, x, w_dw, dx, d, total4);
    TNET_LAUNCH_CHECK("dw bwd data")
    return GHN3_OK;
}

// Steps 2 - 4 of the backward, shared by the family's three members (NORM_NONE: dz = dout; z, stats, gamma, s12 are null and not
// read.  NORM_FROZEN: z and s12 are null and not read): dy = dz W_pw, dW_pw, dx and dW_dw.
template <int NORM>
int dwpw_bwd_products(const Desc& d, const Plan& pl, const float* dout, const float* z, const float* stats, const float* gamma,
                      const float* s12, const float* x, const float* w_dw, const float* w_pw, float* dx, float* dw_dw, float* dw_pw,
                      float* dy, float* part_pw, float* part_dw, hipStream_t s) {
    int rc;
    // 2. dy = dz W_pw
    {
        const int NT = nt_of(d.C_in);
        const size_t lds = bwd_lds(NT);
#define BWD_CASE(n) case n: rc = tnet_raise_lds(tnet_dwpw_bwd_data_kernel<n, NORM>, lds); if (rc) return rc; \
        hipLaunchKernelGGL((tnet_dwpw_bwd_data_kernel<n, NORM>), dim3(pl.n_tiles), dim3(256), lds, s, dout, z, stats, gamma, s12, w_pw, dy, d, pl.P); break;
        switch (NT) { BWD_CASE(4) BWD_CASE(8) BWD_CASE(16) BWD_CASE(32) }
#undef BWD_CASE
        TNET_LAUNCH_CHECK("dwpw bwd data")
    }
    // 3. dW_pw
    hipLaunchKernelGGL(tnet_pw_wgrad_kernel<NORM>, dim3(pl.pw_chunks, (d.C_out + 63) / 64, (d.C_in + 63) / 64), dim3(256), 0, s, dout, z, stats,
                       gamma, s12, x, w_dw, part_pw, d, pl.P, pl.pw_chunk_px);
    TNET_LAUNCH_CHECK("pw wgrad")
    rc = reduce_rows(part_pw, pl.pw_chunks, (int64_t)d.C_out * d.C_in, dw_pw, 0, 0, s, "pw wgrad reduce");
    if (rc) return rc;
    // 4. dx and dW_dw
    rc = dw_bwd_data(d, dy, x, w_dw, dx, s);
    if (rc || !w_dw) return rc;
    return dw_wgrad(d, pl, dy, x, part_dw, dw_dw, s);
}

// (mean, var) of a frozen norm layer -> (mean, rstd) in `stats` [2 C]
int frozen_stats(const float* mean, const float* var, float eps, int C, float* stats, hipStream_t s) {
    hipLaunchKernelGGL(tnet_bn_frozen_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, s, mean, var, eps, C, stats);
    TNET_LAUNCH_CHECK("bn frozen stats")
    return GHN3_OK;
}

// The scratch buffer of a member of the dwpw family (`norm` = NORM_NONE, NORM_BATCH or NORM_FROZEN) in one direction: where each
// area starts, in floats, and the size the caller allocates.  THE one description of the layout: the size functions return
// `total`, the entry points read the offsets; an area a member does not have stays at 0 and is not used.
//   forward   batch: part12 = per tile (mean, M2); the other members need no scratch (total 0)
//   backward  part12 = per tile (sum dout, sum dout xhat), s12 = their reduction when dbeta / dgamma cannot take it in place
//             (members with a norm layer); stats = (mean, rstd) of the frozen statistics; dy; the two weight gradients' partials
struct DwpwScratch { int64_t part12, s12, stats, dy, part_pw, part_dw, total; };

inline int64_t part_dw_floats(const Desc& d, const Plan& pl) { return (int64_t)pl.dw_chunks * d.ks * d.ks * d.C_in; }

DwpwScratch dwpw_scratch(const Desc& d, const Plan& pl, int norm, bool backward) {
    DwpwScratch sc = {};
    int64_t at = 0;
    auto take = [&at](int64_t n) { const int64_t o = at; at += n; return o; };
    if (!backward) {
        if (norm != NORM_BATCH) return sc;
        sc.part12 = take((int64_t)pl.n_tiles * 2 * d.C_out);
        sc.total = at + 64;
        return sc;
    }
    if (norm != NORM_NONE) {
        sc.part12 = take((int64_t)pl.n_tiles * 2 * d.C_out);
        sc.s12 = take(2 * d.C_out);
    }
    if (norm == NORM_FROZEN) sc.stats = take(2 * d.C_out);
    sc.dy = take((int64_t)pl.P * d.C_in);
    sc.part_pw = take((int64_t)pl.pw_chunks * d.C_out * d.C_in);
    sc.part_dw = take(part_dw_floats(d, pl));
    sc.total = at + 256;
    return sc;
}

// what the three size functions of the fused chain answer: -1 for every descriptor the op refuses (ghn3_last_error has the reason)
int64_t dwpw_scratch_floats(const ghn3_dwpw_desc* g, int norm, int backward) {
    Desc d;
    if (check_desc(g, d)) return -1;
    return dwpw_scratch(d, make_plan(d), norm, backward != 0).total;
}

// without depthwise weights the chain is ReLU -> 1x1 convolution: `op` = how the message of the entry point words that
int check_w_dw(const Desc& d, const float* w_dw, const char* op) {
    if (w_dw || (d.ks == 1 && d.pad == 0)) return GHN3_OK;
    ghn3_set_error("dwpw: without depthwise weights %sks = 1, pad = 0", op);
    return GHN3_E_ARG;
}

// The forward kernel of the family -- its only launch.  NORM_BATCH: pre-norm activations to z, per-tile statistics to `part`.
// NORM_NONE: the accumulators are the result, stored to `out`.  NORM_FROZEN: the affine map of (gamma, beta, mean, var) in the
// epilogue, the result to `out`, z beside it when non-null.  What a member does not have is not passed on.
template <int NORM>
int dwpw_fwd_launch(const Desc& d, const Plan& pl, const float* x, const float* w_dw, const float* w_pw, const float* gamma,
                    const float* beta, const float* mean, const float* var, float* z, float* out, float* part, hipStream_t s,
                    const char* what) {
    const int NT = nt_of(d.C_out);
    const size_t lds = fwd_lds(NT, NORM == NORM_BATCH);
    float* const dst = NORM == NORM_NONE ? out : z;
    float* const tiles = NORM == NORM_BATCH ? part : nullptr;
    const Frozen fz = NORM == NORM_FROZEN ? Frozen{gamma, beta, mean, var, out} : Frozen{};
    int rc;
#define FWD_CASE(n) case n: rc = tnet_raise_lds(tnet_dwpw_fwd_kernel<n, NORM>, lds); if (rc) return rc; \
        hipLaunchKernelGGL((tnet_dwpw_fwd_kernel<n, NORM>), dim3(pl.n_tiles), dim3(256), lds, s, x, w_dw, w_pw, dst, tiles, d, pl.P, fz); break;
    switch (NT) { FWD_CASE(4) FWD_CASE(8) FWD_CASE(16) FWD_CASE(32) }
#undef FWD_CASE
    return launched(what);
}

// The forward of a member: `who` names it in the messages, `required` = none of the pointers it needs is null (w_dw is optional
// for every member; the norm's arguments are null for the members without them).
template <int NORM>
int dwpw_fwd_core(const ghn3_dwpw_desc* g, const char* who, bool required, const float* x, const float* w_dw, const float* w_pw,
                  const float* gamma, const float* beta, const float* mean, const float* var, float* z, float* out, float* stats,
                  float* scratch, void* stream_) {
    Desc d;
    int rc = check_desc(g, d);
    if (rc) return rc;
    if (!required) { ghn3_set_error("%s: null pointer", who); return GHN3_E_ARG; }
    rc = check_w_dw(d, w_dw, NORM == NORM_NONE ? "the op is ReLU -> 1x1 conv: " : "the op is ReLU -> 1x1 conv -> norm: ");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream_;
    const Plan pl = make_plan(d);
    float* const part = NORM == NORM_BATCH ? scratch + dwpw_scratch(d, pl, NORM, false).part12 : nullptr;
    rc = dwpw_fwd_launch<NORM>(d, pl, x, w_dw, w_pw, gamma, beta, mean, var, z, out, part, s, who);
    if (rc || NORM != NORM_BATCH) return rc;
    return bn_apply_launch(part, pl.n_tiles, pl.P, d.C_out, d.eps, z, gamma, beta, stats, out, s);
}

// The backward of a member.  Batch statistics: `stats` is the forward's; frozen: (mean, var) -> (mean, rstd) in scratch first.
// Then 1. dgamma / dbeta (members with a norm layer) and 2 - 4. dwpw_bwd_products.
template <int NORM>
int dwpw_bwd_core(const ghn3_dwpw_desc* g, const char* who, bool required, const float* dout, const float* x, const float* z,
                  const float* stats, const float* w_dw, const float* w_pw, const float* gamma, const float* mean, const float* var,
                  float* dx, float* dw_dw, float* dw_pw, float* dgamma, float* dbeta, float* scratch, void* stream_) {
    Desc d;
    int rc = check_desc(g, d);
    if (rc) return rc;
    if (!required || (w_dw && !dw_dw)) { ghn3_set_error("%s: null pointer", who); return GHN3_E_ARG; }
    rc = check_w_dw(d, w_dw, "");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream_;
    const Plan pl = make_plan(d);
    const DwpwScratch sc = dwpw_scratch(d, pl, NORM, true);
    const float* s12 = nullptr;
    if (NORM == NORM_FROZEN) {
        rc = frozen_stats(mean, var, d.eps, d.C_out, scratch + sc.stats, s);
        if (rc) return rc;
        stats = scratch + sc.stats;
    }
    if (NORM != NORM_NONE) {
        rc = bn_param_grads(dout, z, stats, scratch + sc.part12, scratch + sc.s12, dgamma, dbeta, pl.n_tiles, pl.P, d.C_out, s, &s12);
        if (rc) return rc;
    }
    // (dz: batch statistics read z and the reduced pair, frozen ones neither)
    return dwpw_bwd_products<NORM>(d, pl, dout, NORM == NORM_BATCH ? z : nullptr, stats, gamma, NORM == NORM_BATCH ? s12 : nullptr, x, w_dw,
                                   w_pw, dx, dw_dw, dw_pw, scratch + sc.dy, scratch + sc.part_pw, scratch + sc.part_dw, s);
}

}  // namespace

// The three size functions of the fused chain answer -1 (= GHN3_E_ARG) for EVERY refusal, a limit included; ghn3_dw_scratch_floats
// and the dense-convolution pair answer the GHN3_E_* code of the refusal.
extern "C" int64_t ghn3_dwpw_scratch_floats(const ghn3_dwpw_desc* g, int backward) { return dwpw_scratch_floats(g, NORM_BATCH, backward); }

extern "C" int ghn3_dwpw_bn_fwd(const ghn3_dwpw_desc* g, const float* x, const float* w_dw, const float* w_pw, const float* gamma,
                                const float* beta, float* z, float* out, float* stats, float* scratch, void* stream_) {
    return dwpw_fwd_core<NORM_BATCH>(g, "dwpw fwd", x && w_pw && gamma && beta && z && out && stats && scratch, x, w_dw, w_pw, gamma, beta,
                                     nullptr, nullptr, z, out, stats, scratch, stream_);
}

extern "C" int ghn3_dwpw_bn_bwd(const ghn3_dwpw_desc* g, const float* dout, const float* x, const float* z, const float* stats,
                                const float* w_dw, const float* w_pw, const float* gamma, float* dx, float* dw_dw, float* dw_pw,
                                float* dgamma, float* dbeta, float* scratch, void* stream_) {
    return dwpw_bwd_core<NORM_BATCH>(g, "dwpw bwd", dout && x && z && stats && w_pw && gamma && dx && dw_pw && dgamma && dbeta && scratch,
                                     dout, x, z, stats, w_dw, w_pw, gamma, nullptr, nullptr, dx, dw_dw, dw_pw, dgamma, dbeta, scratch, stream_);
}

// ---- the same family without a norm layer: out = pw(dw(relu(x))) -- the blocks of a norm=None network (ops.py:91-96) -----------
// Forward: the forward kernel alone, its accumulators stored straight to `out` (no z, no statistics, no scratch).  Backward: dz IS
// dout, so steps 2 - 4 of the backward above run on dout directly; nothing of activation size but x is kept between the two.
extern "C" int64_t ghn3_dwpw_plain_scratch_floats(const ghn3_dwpw_desc* g, int backward) { return dwpw_scratch_floats(g, NORM_NONE, backward); }

extern "C" int ghn3_dwpw_plain_fwd(const ghn3_dwpw_desc* g, const float* x, const float* w_dw, const float* w_pw, float* out,
                                   void* stream_) {
    return dwpw_fwd_core<NORM_NONE>(g, "dwpw plain fwd", x && w_pw && out, x, w_dw, w_pw, nullptr, nullptr, nullptr, nullptr, nullptr, out,
                                    nullptr, nullptr, stream_);
}

extern "C" int ghn3_dwpw_plain_bwd(const ghn3_dwpw_desc* g, const float* dout, const float* x, const float* w_dw, const float* w_pw,
                                   float* dx, float* dw_dw, float* dw_pw, float* scratch, void* stream_) {
    return dwpw_bwd_core<NORM_NONE>(g, "dwpw plain bwd", dout && x && w_pw && dx && dw_pw && scratch, dout, x, nullptr, nullptr, w_dw, w_pw,
                                    nullptr, nullptr, nullptr, dx, dw_dw, dw_pw, nullptr, nullptr, scratch, stream_);
}

// ---- the same family behind a norm layer with FROZEN statistics: out = (pw(dw(relu(x))) - mean) rstd gamma + beta, rstd = 1 /
// sqrt(var + eps) -- the blocks of a network whose BatchNorm layers normalise with their running statistics (eval mode) ----------
// Forward: the forward kernel alone (NORM_FROZEN): the affine map in its epilogue, z stored beside out only when the caller
// wants a backward.  Backward: (mean, var) -> (mean, rstd) once, dgamma / dbeta as with batch statistics, then steps 2 - 4 on
// dz = dout gamma rstd formed on the fly.  The statistics are read only.
extern "C" int64_t ghn3_dwpw_frozen_scratch_floats(const ghn3_dwpw_desc* g, int backward) { return dwpw_scratch_floats(g, NORM_FROZEN, backward); }

extern "C" int ghn3_dwpw_frozen_fwd(const ghn3_dwpw_desc* g, const float* x, const float* w_dw, const float* w_pw, const float* gamma,
                                    const float* beta, const float* mean, const float* var, float* z, float* out, void* stream_) {
    return dwpw_fwd_core<NORM_FROZEN>(g, "dwpw frozen fwd", x && w_pw && gamma && beta && mean && var && out, x, w_dw, w_pw, gamma, beta, mean,
                                      var, z, out, nullptr, nullptr, stream_);
}

extern "C" int ghn3_dwpw_frozen_bwd(const ghn3_dwpw_desc* g, const float* dout, const float* x, const float* z, const float* w_dw,
                                    const float* w_pw, const float* gamma, const float* mean, const float* var, float* dx, float* dw_dw,
                                    float* dw_pw, float* dgamma, float* dbeta, float* scratch, void* stream_) {
    return dwpw_bwd_core<NORM_FROZEN>(g, "dwpw frozen bwd",
                                      dout && x && z && w_pw && gamma && mean && var && dx && dw_pw && dgamma && dbeta && scratch, dout, x, z,
                                      nullptr, w_dw, w_pw, gamma, mean, var, dx, dw_dw, dw_pw, dgamma, dbeta, scratch, stream_);
}

// ---- the depthwise stage ALONE: y = depthwise(relu(x)) -- the first of the two nodes a ReLU -> depthwise -> pointwise -> norm
// chain runs as when it is wider than the fused kernels take (max(C_in, C_out) > 512: tnet_dwpw_fwd_kernel keeps all output columns
// of a pixel tile in one workgroup's accumulators); the pointwise convolution and the norm then run on the dense-convolution
// family, whose kernels split the columns over the grid.  Same descriptor with C_out == C_in; C a multiple of 4, C <= 16384.
// Forward: one launch, no scratch.  Backward: dx (tnet_dw_bwd_data_kernel) and dW_dw (tnet_dw_wgrad_kernel + reduction) from
// dout directly: 3 launches; scratch = the weight gradient's partials.
namespace {

constexpr int DW_CS = 128;       // channels per workgroup of the forward (32 quads x 8 pixel lanes)
constexpr int DW_PX = 32;        // output pixels per workgroup

// workgroup = (DW_PX output pixels, DW_CS channels): the slice's taps in LDS ([tap][channel], read as four floats), thread =
// (channel quad, pixel lane): 16-byte loads, a wave reads 512 consecutive bytes of two pixels per tap; taps in (kh, kw) order.
__global__ __launch_bounds__(256) void tnet_dw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w_dw,
                                                          float* __restrict__ y, const Desc d, const int P) {
    __shared__ __attribute__((aligned(16))) float wt[MAXT * DW_CS];
    const int c0 = blockIdx.y * DW_CS, nc = min(DW_CS, d.C_in - c0), taps = d.ks * d.ks;
    for (int i = threadIdx.x; i < taps * DW_CS; i += 256) {
        const int t = i / DW_CS, cc = i - t * DW_CS;
        wt[i] = cc < nc ? w_dw[(int64_t)(c0 + cc) * taps + t] : 0.f;
    }
    __syncthreads();
    const int cq = threadIdx.x & 31, pl = threadIdx.x >> 5;
    if (4 * cq >= nc) return;
    const int c = c0 + 4 * cq, hw = d.Ho * d.Wo;
    const int pa = blockIdx.x * DW_PX, pb = min(P, pa + DW_PX);
    for (int p = pa + pl; p < pb; p += 8) {
        const int n = p / hw, r = p - n * hw, oh = r / d.Wo, ow = r - oh * d.Wo;
        const int ih0 = oh * d.stride - d.pad, iw0 = ow * d.stride - d.pad;
        const float* xn = x + (int64_t)n * d.H * d.W * d.C_in + c;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        int t = 0;
        for (int kh = 0; kh < d.ks; ++kh) {
            const int ih = ih0 + kh * d.dil;
            for (int kw = 0; kw < d.ks; ++kw, ++t) {
                const int iw = iw0 + kw * d.dil;
                if (ih < 0 || ih >= d.H || iw < 0 || iw >= d.W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(xn + ((int64_t)ih * d.W + iw) * d.C_in);
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wt + t * DW_CS + 4 * cq);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(fmaxf(v[e], 0.f), wv[e], acc[e]);
            }
        }
        *reinterpret_cast<f32x4*>(y + (int64_t)p * d.C_in + c) = acc;
    }
}

// check_desc with the rules of the stand-alone op
inline int check_dw_desc(const ghn3_dwpw_desc* g, Desc& d) { return check_desc(g, d, "dw", DW_MAX_C, true); }

}  // namespace

// (scratch: the weight gradient's partials alone, at offset 0)
extern "C" int64_t ghn3_dw_scratch_floats(const ghn3_dwpw_desc* g, int backward) {
    Desc d;
    const int rc = check_dw_desc(g, d);
    if (rc) return rc;                                            // GHN3_E_ARG / GHN3_E_LIMIT
    return backward ? part_dw_floats(d, make_plan(d)) + 256 : 0;
}

extern "C" int ghn3_dw_fwd(const ghn3_dwpw_desc* g, const float* x, const float* w_dw, float* y, void* stream_) {
    Desc d;
    const int rc = check_dw_desc(g, d);
    if (rc) return rc;
    if (!x || !w_dw || !y) { ghn3_set_error("dw fwd: null pointer"); return GHN3_E_ARG; }
    const int P = d.N * d.Ho * d.Wo;
    hipLaunchKernelGGL(tnet_dw_fwd_kernel, dim3((P + DW_PX - 1) / DW_PX, (d.C_in + DW_CS - 1) / DW_CS), dim3(256), 0, (hipStream_t)stream_,
                       x, w_dw, y, d, P);
    TNET_LAUNCH_CHECK("dw fwd")
    return GHN3_OK;
}

extern "C" int ghn3_dw_bwd(const ghn3_dwpw_desc* g, const float* dout, const float* x, const float* w_dw, float* dx, float* dw_dw,
                           float* scratch, void* stream_) {
    Desc d;
    int rc = check_dw_desc(g, d);
    if (rc) return rc;
    if (!dout || !x || !w_dw || !dx || !dw_dw || !scratch) { ghn3_set_error("dw bwd: null pointer"); return GHN3_E_ARG; }
    hipStream_t s = (hipStream_t)stream_;
    rc = dw_bwd_data(d, dout, x, w_dw, dx, s);
    if (rc) return rc;
    return dw_wgrad(d, make_plan(d), dout, x, scratch, dw_dw, s);
}

// ---- dense convolution family: the forward / input-gradient kernel and the host side -------------------------------------------
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// The implicit GEMM of the dense convolution, three bf16 pieces per operand:
//  * the weight pieces are cut ONCE per call (tnet_conv_w_pack_kernel: [piece][tap][row][k], k padded to the chunk), so the B tile
//    of a chunk is a plain 16-byte copy;
//  * the output columns are split over blockIdx.y (NT <= 8 fragments per workgroup): the small-image / wide-layer shapes of the
//    search space (4 x 4 x 256 channels: 16 pixel tiles) fill the chip;
//  * global loads of chunk i + 1 are in flight during the matrix products of chunk i (registers -> the other LDS buffer: one
//    barrier per chunk), the A pieces are stored as 16-byte vectors;
//  * the backward reads dz from a buffer written once (tnet_dz_kernel).
// BWD = false: dst = z[P_dst = output pixels][R = C_out] from src = x;  BWD = true: dst = dx[input pixels][R = C_in] from src = dz.
// EPI, what the forward does with its accumulators (the backward has EPI_STATS and stores dx alone):
//  * EPI_STATS: dst = z and the per-tile (mean, M2) of every channel to `part`;
//  * EPI_FROZEN: the norm layer behind the convolution has frozen statistics: its affine map is applied to the accumulators and
//    stored to ep.fz.out, dst = z is stored as well when it is non-null, and the kernel ends there (no statistics);
//  * EPI_BIAS (the "bias" member): ep.fz.out = act(acc + ep.bias[c] [+ ep.res]), act = ReLU when ep.act else the identity; dst and
//    `part` are not touched, nothing else is stored.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tnet_conv_w_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ wp, int C_out,
                                                               int C_in, int taps, int transposed) {
    const int R = transposed ? C_in : C_out, K = transposed ? C_out : C_in, Kp = (K + KC - 1) / KC * KC;
    const int64_t plane = (int64_t)taps * R * Kp;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < plane; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i % Kp);
        const int64_t tr = i / Kp;
        const int r = (int)(tr % R), t = (int)(tr / R);
        float v = 0.f;
        if (k < K) {
            const int co = transposed ? k : r, ci = transposed ? r : k;
            v = w[((int64_t)co * C_in + ci) * taps + t];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const unsigned short h = bf16_rn(v);
            wp[q * plane + i] = h;
            v -= __uint_as_float((unsigned)h << 16);
        }
    }
}

// dz [P][C] of a norm layer, written once.  BATCH = false: frozen statistics, dz = gamma rstd dout (z and s12 are not touched).
template <bool BATCH = true>
__global__ __launch_bounds__(256) void tnet_dz_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                      const float* __restrict__ stats, const float* __restrict__ gamma,
                                                      const float* __restrict__ s12, float* __restrict__ dz, int64_t total4, int C, int P) {
    const float invP = 1.f / (float)P;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % C);
        const f32x4 g = *reinterpret_cast<const f32x4*>(dout + 4 * i);
        const f32x4 rs = *reinterpret_cast<const f32x4*>(stats + C + c), ga = *reinterpret_cast<const f32x4*>(gamma + c);
        f32x4 o;
        if constexpr (BATCH) {
            const f32x4 zz = *reinterpret_cast<const f32x4*>(z + 4 * i), mu = *reinterpret_cast<const f32x4*>(stats + c);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(s12 + c), a2 = *reinterpret_cast<const f32x4*>(s12 + C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (zz[e] - mu[e]) * rs[e];
                o[e] = ga[e] * rs[e] * (g[e] - a1[e] * invP - xh * a2[e] * invP);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ga[e] * rs[e] * g[e];
        }
        *reinterpret_cast<f32x4*>(dz + 4 * i) = o;
    }
}

// dz of the "act" member: tnet_dz_kernel on g = dout 1[out > 0], the mask applied as dout is read; the same pass writes the
// skip tensor's gradient dres = g when dres is non-null.  s12 holds the sums of the MASKED gradient (tnet_bn_act_bwd_partial_kernel).
template <bool BATCH = true>
__global__ __launch_bounds__(256) void tnet_dz_act_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                          const float* __restrict__ z, const float* __restrict__ stats,
                                                          const float* __restrict__ gamma, const float* __restrict__ s12,
                                                          float* __restrict__ dz, float* __restrict__ dres, int64_t total4, int C, int P) {
    const float invP = 1.f / (float)P;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % C);
        const f32x4 g = act_masked(*reinterpret_cast<const f32x4*>(dout + 4 * i), *reinterpret_cast<const f32x4*>(out + 4 * i));
        if (dres) *reinterpret_cast<f32x4*>(dres + 4 * i) = g;
        const f32x4 rs = *reinterpret_cast<const f32x4*>(stats + C + c), ga = *reinterpret_cast<const f32x4*>(gamma + c);
        f32x4 o;
        if constexpr (BATCH) {
            const f32x4 zz = *reinterpret_cast<const f32x4*>(z + 4 * i), mu = *reinterpret_cast<const f32x4*>(stats + c);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(s12 + c), a2 = *reinterpret_cast<const f32x4*>(s12 + C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (zz[e] - mu[e]) * rs[e];
                o[e] = ga[e] * rs[e] * (g[e] - a1[e] * invP - xh * a2[e] * invP);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ga[e] * rs[e] * g[e];
        }
        *reinterpret_cast<f32x4*>(dz + 4 * i) = o;
    }
}

constexpr int EPI_STATS = 0, EPI_FROZEN = 1, EPI_BIAS = 2;

// The epilogue's operands: the frozen norm layer's constants and the result's address (EPI_FROZEN; EPI_BIAS uses fz.out alone),
// the bias [C_out], the skip tensor [P][C_out] or null, and whether the result is clamped at zero (EPI_BIAS).
struct ConvEpi {
    Frozen fz;
    const float *bias, *res;
    int act;
};

template <int NT, bool BWD, int EPI = EPI_STATS>
__global__ __launch_bounds__(256) void tnet_conv2_kernel(const float* __restrict__ src, const unsigned short* __restrict__ wp,
                                                         float* __restrict__ dst, float* __restrict__ part,
                                                         const float* __restrict__ xmask, const CDesc d, const int P_dst, const int P_src,
                                                         const ConvEpi ep) {
    static_assert(!(BWD && EPI != EPI_STATS), "the epilogues are the forward's");
    constexpr int S = 3;
    constexpr int A_BUF = S * TP * LDK, B_BUF = S * 16 * NT * LDK;             // 16-bit elements per stage
    constexpr int NB = (S * 16 * NT * 4 + 255) / 256;                          // 16-byte units of the B tile per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* pix = reinterpret_cast<int*>(smem);                                   // [3][TP]
    unsigned short* As = reinterpret_cast<unsigned short*>(smem + 3 * TP * 4); // [2][S][TP][LDK]
    unsigned short* Bs = As + 2 * A_BUF;                                       // [2][S][16 NT][LDK]
    float* red = reinterpret_cast<float*>(As);                                 // epilogue (forward statistics): [5][16 NT], aliased
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, kc = lane >> 4;
    const int tile = blockIdx.x, p0 = tile * TP, taps = d.kh * d.kw, col0 = blockIdx.y * 16 * NT;
    const int R = BWD ? d.C_in : d.C_out, K = BWD ? d.C_out : d.C_in, Kp = (K + KC - 1) / KC * KC, nchunk = Kp / KC;
    const int64_t plane = (int64_t)taps * R * Kp;
    if (tid < TP) {
        const int p = p0 + tid;
        int n = -1, a = 0, b = 0;
        if (p < P_dst) {
            if (BWD) {
                const int hw = d.H * d.W;
                n = p / hw;
                const int r = p - n * hw, ih = r / d.W, iw = r - ih * d.W;
                a = ih + d.ph; b = iw + d.pw;
            } else {
                const int hw = d.Ho * d.Wo;
                n = p / hw;
                const int r = p - n * hw, oh = r / d.Wo, ow = r - oh * d.Wo;
                a = oh * d.sh - d.ph; b = ow * d.sw - d.pw;
            }
        }
        pix[tid] = n; pix[TP + tid] = a; pix[2 * TP + tid] = b;
    }
    __syncthreads();
    const int ai = tid >> 2, acc_ = (tid & 3) * 8;                             // this thread's A row (pixel) and k offset
    const int an = pix[ai], aa = pix[TP + ai], ab = pix[2 * TP + ai];
    f32x4 a0, a1;                                                              // prefetched A values (8 floats)
    u16x8 breg[NB];                                                            // prefetched B units
    auto fetch = [&](int it) {
        const int t = it / nchunk, c0 = (it - t * nchunk) * KC;
        const int dh = (t / d.kw) * d.dil, dw_ = (t % d.kw) * d.dil;
        int64_t ps = -1;
        if (an >= 0) {
            if (BWD) {
                const int th = aa - dh, tw = ab - dw_;
                if (th >= 0 && tw >= 0 && th % d.sh == 0 && tw % d.sw == 0) {
                    const int oh = th / d.sh, ow = tw / d.sw;
                    if (oh < d.Ho && ow < d.Wo) ps = ((int64_t)an * d.Ho + oh) * d.Wo + ow;
                }
            } else {
                const int ih = aa + dh, iw = ab + dw_;
                if (ih >= 0 && ih < d.H && iw >= 0 && iw < d.W) ps = ((int64_t)an * d.H + ih) * d.W + iw;
            }
        }
        const int c = c0 + acc_;
        a0 = f32x4{0.f, 0.f, 0.f, 0.f}; a1 = a0;
        if (ps >= 0 && c < K) {
            const float* px = src + ps * K + c;
            a0 = *reinterpret_cast<const f32x4*>(px);
            if (c + 4 < K) a1 = *reinterpret_cast<const f32x4*>(px + 4);
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int i = tid + 256 * u;                                       // unit index: [piece][row][4 segments]
            const int q = i / (64 * NT), r = (i - q * 64 * NT) >> 2, seg = i & 3;
            u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (i < S * 64 * NT && col0 + r < R)
                v = *reinterpret_cast<const u16x8*>(wp + q * plane + ((int64_t)t * R + col0 + r) * Kp + c0 + 8 * seg);
            breg[u] = v;
        }
    };
    auto stage = [&](int buf) {                                                // registers -> LDS stage `buf`
        unsigned short* A = As + buf * A_BUF;
        unsigned short* B = Bs + buf * B_BUF;
        float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        if (!BWD && d.relu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
        }
#pragma unroll
        for (int q = 0; q < S; ++q) {
            unsigned h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                h[e] = bf16_pk(v[2 * e], v[2 * e + 1]);
                v[2 * e] -= __uint_as_float(h[e] << 16);
                v[2 * e + 1] -= __uint_as_float(h[e] & 0xffff0000u);
            }
            *reinterpret_cast<uint4*>(A + q * TP * LDK + ai * LDK + acc_) = uint4{h[0], h[1], h[2], h[3]};
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int i = tid + 256 * u;
            const int q = i / (64 * NT), r = (i - q * 64 * NT) >> 2, seg = i & 3;
            if (i < S * 64 * NT) *reinterpret_cast<u16x8*>(B + q * 16 * NT * LDK + r * LDK + 8 * seg) = breg[u];
        }
    };
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int n_it = taps * nchunk;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int it = 0; it < n_it; ++it) {
        const int buf = it & 1;
        if (it + 1 < n_it) fetch(it + 1);                                      // (in flight during the products below)
        {
            const unsigned short* A = As + buf * A_BUF;
            const unsigned short* B = Bs + buf * B_BUF;
            u16x8 af[S];
#pragma unroll
            for (int q = 0; q < S; ++q) af[q] = frag(A + q * TP * LDK, 16 * w + r16, kc);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                u16x8 bf[S];
#pragma unroll
                for (int q = 0; q < S; ++q) bf[q] = frag(B + q * 16 * NT * LDK, 16 * j + r16, kc);
                acc[j] = mma_terms<S>(af, bf, acc[j]);
            }
        }
        if (it + 1 < n_it) stage(buf ^ 1);
        __syncthreads();
    }
    const int prow = p0 + 16 * w + r16;
    const bool valid = prow < P_dst;
    if constexpr (EPI == EPI_FROZEN) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = col0 + 16 * j + 4 * kc;
            if (valid && col < R) {
                if (dst) *reinterpret_cast<f32x4*>(dst + (int64_t)prow * R + col) = acc[j];
                *reinterpret_cast<f32x4*>(ep.fz.out + (int64_t)prow * R + col) = frozen_affine4(acc[j], ep.fz, col, d.eps);
            }
        }
        return;
    }
    if constexpr (EPI == EPI_BIAS) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = col0 + 16 * j + 4 * kc;
            if (valid && col < R) {
                f32x4 v = acc[j] + *reinterpret_cast<const f32x4*>(ep.bias + col);
                if (ep.res) v += *reinterpret_cast<const f32x4*>(ep.res + (int64_t)prow * R + col);
                if (ep.act) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                *reinterpret_cast<f32x4*>(ep.fz.out + (int64_t)prow * R + col) = v;
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = col0 + 16 * j + 4 * kc;
        if (valid && col < R) {
            f32x4 v = acc[j];
            if (BWD && d.relu) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xmask + (int64_t)prow * R + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = xv[e] > 0.f ? v[e] : 0.f;
            }
            *reinterpret_cast<f32x4*>(dst + (int64_t)prow * R + col) = v;
        }
    }
    if (BWD) return;
    // ---- forward: per-tile (mean, M2) of every channel of this column group (as tnet_dwpw_fwd_kernel)
    const int cnt = min(TP, P_dst - p0);
    auto tile_sum = [&](bool centred) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = 16 * j + 4 * kc;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = 0.f;
                if (valid) { v = acc[j][e]; if (centred) { v -= red[4 * 16 * NT + col + e]; v *= v; } }
                v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
                if (r16 == 0) red[w * 16 * NT + col + e] = v;
            }
        }
        __syncthreads();
    };
    tile_sum(false);
    for (int c = tid; c < 16 * NT; c += 256)
        red[4 * 16 * NT + c] = (red[c] + red[16 * NT + c] + red[2 * 16 * NT + c] + red[3 * 16 * NT + c]) / (float)cnt;
    tile_sum(true);
    for (int c = tid; c < 16 * NT; c += 256) {
        if (col0 + c < R) {
            part[((int64_t)tile * 2) * R + col0 + c] = red[4 * 16 * NT + c];
            part[((int64_t)tile * 2 + 1) * R + col0 + c] = red[c] + red[16 * NT + c] + red[2 * 16 * NT + c] + red[3 * 16 * NT + c];
        }
    }
}

constexpr int CONV_MAX_IN = 16384, CONV_MAX_OUT = 4096;

struct CPlan { int P, P_in, n_tiles, n_tiles_in, w_chunks, w_chunk_px, taps; };

CPlan make_cplan(const CDesc& d) {
    CPlan pl;
    pl.taps = d.kh * d.kw;
    pl.P = d.N * d.Ho * d.Wo;
    pl.P_in = d.N * d.H * d.W;
    pl.n_tiles = (pl.P + TP - 1) / TP;
    pl.n_tiles_in = (pl.P_in + TP - 1) / TP;
    const int blocks = ((d.C_out + 63) / 64) * ((d.C_in + 63) / 64) * pl.taps;
    int chunks = (768 + blocks - 1) / blocks;
    chunks = std::max(1, std::min(chunks, (pl.P + KC - 1) / KC));
    pl.w_chunk_px = ((pl.P + chunks - 1) / chunks + KC - 1) / KC * KC;
    pl.w_chunks = (pl.P + pl.w_chunk_px - 1) / pl.w_chunk_px;
    return pl;
}

int check_cdesc(const ghn3_conv_desc* g, CDesc& d) {
    if (!g) { ghn3_set_error("conv: null descriptor"); return GHN3_E_ARG; }
    d = CDesc{g->N, g->H, g->W, g->C_in, g->C_out, g->kh, g->kw, g->stride_h, g->stride_w, g->pad_h, g->pad_w, g->dil, g->Ho, g->Wo,
              (g->relu & 1) != 0, g->eps};
    if (d.N <= 0 || d.H <= 0 || d.W <= 0 || d.C_in <= 0 || d.C_out <= 0 || d.kh <= 0 || d.kw <= 0 || d.sh <= 0 || d.sw <= 0 ||
        d.dil <= 0 || d.ph < 0 || d.pw < 0) {
        ghn3_set_error("conv: non-positive size in the descriptor");
        return GHN3_E_ARG;
    }
    // (tnet_conv2_kernel walks the reduction in chunks and splits the columns over blockIdx.y in both directions, the weight
    // gradient tiles both sides over the grid, the norm kernels loop over the channels: wide layers are fine)
    if ((d.C_in & 3) || (d.C_out & 3) || d.C_in > CONV_MAX_IN || d.C_out > CONV_MAX_OUT || d.kh > 7 || d.kw > 7) {
        ghn3_set_error("conv: needs C_in, C_out multiples of 4, C_out <= %d, C_in <= %d, kernel <= 7 x 7 (got %d -> %d, %d x %d)",
                       CONV_MAX_OUT, CONV_MAX_IN, d.C_in, d.C_out, d.kh, d.kw);
        return GHN3_E_LIMIT;
    }
    // (the weight gradient's reduction runs four threads per weight on a one-dimensional grid)
    if ((int64_t)d.kh * d.kw * d.C_out * d.C_in >= ((int64_t)1 << 30)) {
        ghn3_set_error("conv: weight tensors of 2^30 elements or more are not supported");
        return GHN3_E_LIMIT;
    }
    const int ho = (d.H + 2 * d.ph - d.dil * (d.kh - 1) - 1) / d.sh + 1, wo = (d.W + 2 * d.pw - d.dil * (d.kw - 1) - 1) / d.sw + 1;
    if (ho != d.Ho || wo != d.Wo || ho <= 0 || wo <= 0) {
        ghn3_set_error("conv: output size %d x %d does not match the convolution arithmetic (%d x %d)", d.Ho, d.Wo, ho, wo);
        return GHN3_E_ARG;
    }
    if ((int64_t)d.N * d.H * d.W * std::max(d.C_in, d.C_out) >= ((int64_t)1 << 31) ||
        (int64_t)d.N * d.Ho * d.Wo * std::max(d.C_in, d.C_out) >= ((int64_t)1 << 31)) {
        ghn3_set_error("conv: activation tensors of 2^31 elements or more are not supported");
        return GHN3_E_LIMIT;
    }
    return GHN3_OK;
}

// 16-bit weight pieces, in floats: [3][taps][rows][k padded to the chunk]
inline int64_t pack_floats(int taps, int rows, int k) { return (((int64_t)3 * taps * rows * ((k + KC - 1) / KC * KC) + 1) / 2 + 3) / 4 * 4; }
// columns per workgroup of tnet_conv2_kernel: as wide as possible while the grid still covers the chip
inline int conv2_nt(int tiles, int cols) {
    int nt = cols <= 32 ? 2 : cols <= 64 ? 4 : 8;
    while (nt > 2 && (int64_t)tiles * ((cols + 16 * nt - 1) / (16 * nt)) < 256) nt >>= 1;
    return nt;
}
inline size_t conv2_lds(int NT) { return 3 * TP * 4 + 2 * (3 * TP * LDK + 3 * 16 * NT * LDK) * 2; }

// The scratch buffer of the conv op: where each area starts, in floats (every area a multiple of four), and the size the caller
// allocates.  THE one description of the layout, for both members (`frozen`: behind a norm layer with frozen statistics; the
// convolution alone, GHN3_CONV_NO_NORM, has the layout of the batch member).  Forward: part (not frozen: no statistics), wp.
// Backward: all of them; wp holds the transposed pack; frozen: stats = (mean, rstd), behind the padded layout of the batch member.
struct CScratch { int64_t part, s12, wp, part_w, dz, stats, total; };

CScratch conv_scratch(const CDesc& d, const CPlan& pl, bool frozen, bool backward) {
    CScratch sc = {};
    int64_t at = 0;
    auto take = [&at](int64_t n) { const int64_t o = at; at += n; return o; };
    if (!backward) {
        if (!frozen) sc.part = take((int64_t)pl.n_tiles * 2 * d.C_out);   // per tile: (mean, M2)
        sc.wp = take(pack_floats(pl.taps, d.C_out, d.C_in));
        sc.total = at + 64;
        return sc;
    }
    sc.part = take((int64_t)pl.n_tiles * 2 * d.C_out);             // per tile: (sum dout, sum dout xhat)
    sc.s12 = take(2 * d.C_out);                                    // the reduced pair, when dbeta / dgamma cannot take it in place
    sc.wp = take(pack_floats(pl.taps, d.C_in, d.C_out));
    sc.part_w = take((int64_t)pl.w_chunks * pl.taps * d.C_out * d.C_in);
    sc.dz = take((int64_t)pl.P * d.C_out);
    take(256);
    if (frozen) sc.stats = take(2 * d.C_out);
    sc.total = at;
    return sc;
}

// what the two size functions answer: the GHN3_E_* code of the refusal for a descriptor the op does not take
int64_t conv_scratch_floats(const ghn3_conv_desc* g, bool frozen, int backward) {
    CDesc d;
    const int rc = check_cdesc(g, d);
    if (rc) return rc;                                            // GHN3_E_ARG / GHN3_E_LIMIT
    return conv_scratch(d, make_cplan(d), frozen, backward != 0).total;
}

// Steps 3 and 4 of the backward, shared by every member of the family: dx by the transposed implicit GEMM and dW, both from a
// plain dz [P][C_out] buffer.
int conv_bwd_products(const CDesc& d, const CPlan& pl, const CScratch& sc, const float* dz, const float* x, const float* w, float* dx,
                      float* dw, float* scratch, hipStream_t s) {
    int rc;
    const int64_t wr = (int64_t)pl.taps * d.C_out * d.C_in;
    // 3. dx
    unsigned short* wp = reinterpret_cast<unsigned short*>(scratch + sc.wp);
    const int64_t plane = (int64_t)pl.taps * d.C_in * ((d.C_out + KC - 1) / KC * KC);
    hipLaunchKernelGGL(tnet_conv_w_pack_kernel, grid1d(plane, 2048), dim3(256), 0, s, w, wp, d.C_out, d.C_in, pl.taps, 1);
    TNET_LAUNCH_CHECK("conv weight pack (transposed)")
    const int NT = conv2_nt(pl.n_tiles_in, d.C_in);
    const dim3 grid(pl.n_tiles_in, (d.C_in + 16 * NT - 1) / (16 * NT));
    const size_t lds = conv2_lds(NT);
#define C2B_CASE(n) case n: rc = tnet_raise_lds(tnet_conv2_kernel<n, true>, lds); if (rc) return rc; \
    hipLaunchKernelGGL((tnet_conv2_kernel<n, true>), grid, dim3(256), lds, s, dz, wp, dx, (float*)nullptr, x, d, pl.P_in, pl.P, ConvEpi{}); break;
    switch (NT) { C2B_CASE(2) C2B_CASE(4) C2B_CASE(8) }
#undef C2B_CASE
    TNET_LAUNCH_CHECK("conv bwd data")
    // 4. dW (in the parameter's own [C_out][C_in][kh][kw] order)
    float* part_w = scratch + sc.part_w;
    hipLaunchKernelGGL(tnet_conv_wgrad_kernel, dim3(pl.w_chunks, (d.C_out + 63) / 64, ((d.C_in + 63) / 64) * pl.taps), dim3(256), 0, s, dz, x,
                       part_w, d, pl.P, pl.w_chunk_px);
    TNET_LAUNCH_CHECK("conv wgrad")
    return reduce_rows(part_w, pl.w_chunks, wr, dw, d.C_out * d.C_in, pl.taps, s, "conv wgrad reduce");
}

// The forward convolution of every member: weight pack, then the implicit GEMM.  EPI_STATS: z = the convolution's result, the
// per-tile statistics to the scratch's `part`.  EPI_FROZEN: the affine map of `ep.fz` in the epilogue (ep.fz.out the result, z
// beside it when non-null), no statistics.  EPI_BIAS: ep.fz.out = act(result + bias [+ res]), z not touched, no statistics.
template <int EPI>
int conv_fwd_launch(const CDesc& d, const CPlan& pl, const CScratch& sc, const float* x, const float* w, float* z, const ConvEpi& ep,
                    float* scratch, hipStream_t s, const char* what) {
    float* const part = EPI != EPI_STATS ? nullptr : scratch + sc.part;
    unsigned short* wp = reinterpret_cast<unsigned short*>(scratch + sc.wp);
    const int64_t plane = (int64_t)pl.taps * d.C_out * ((d.C_in + KC - 1) / KC * KC);
    hipLaunchKernelGGL(tnet_conv_w_pack_kernel, grid1d(plane, 2048), dim3(256), 0, s, w, wp, d.C_out, d.C_in, pl.taps, 0);
    TNET_LAUNCH_CHECK("conv weight pack")
    const int NT = conv2_nt(pl.n_tiles, d.C_out);
    const dim3 grid(pl.n_tiles, (d.C_out + 16 * NT - 1) / (16 * NT));
    const size_t lds = conv2_lds(NT);
    int rc;
#define C2F_CASE(n) case n: rc = tnet_raise_lds(tnet_conv2_kernel<n, false, EPI>, lds); if (rc) return rc; \
    hipLaunchKernelGGL((tnet_conv2_kernel<n, false, EPI>), grid, dim3(256), lds, s, x, wp, z, part, (const float*)nullptr, d, pl.P, pl.P_in, ep); break;
    switch (NT) { C2F_CASE(2) C2F_CASE(4) C2F_CASE(8) }
#undef C2F_CASE
    return launched(what);
}

// The backward of every member.  The convolution alone (GHN3_CONV_NO_NORM, not `frozen`): dz = dout.  Batch statistics: dgamma /
// dbeta, then dz written once for the two kernels that read it.  `frozen`: (mean, var) -> (mean, rstd) first, dz = dout gamma rstd.
// `required` = none of the pointers every member needs is null, `norm_required` = nor of those of the norm layer.
int conv_bwd_core(const ghn3_conv_desc* g, bool frozen, const char* who, bool required, bool norm_required, const float* dout, const float* x,
                  const float* z, const float* stats, const float* w, const float* gamma, const float* mean, const float* var, float* dx,
                  float* dw, float* dgamma, float* dbeta, float* scratch, void* stream_) {
    CDesc d;
    int rc = check_cdesc(g, d);
    if (rc) return rc;
    const bool no_norm = (g->relu & GHN3_CONV_NO_NORM) != 0;       // dout IS the gradient of the convolution's result
    if (frozen && no_norm) { ghn3_set_error("conv frozen: GHN3_CONV_NO_NORM has no meaning here"); return GHN3_E_ARG; }
    if (!required || (!no_norm && !norm_required)) { ghn3_set_error("%s: null pointer", who); return GHN3_E_ARG; }
    hipStream_t s = (hipStream_t)stream_;
    const CPlan pl = make_cplan(d);
    const CScratch sc = conv_scratch(d, pl, frozen, true);
    if (no_norm) return conv_bwd_products(d, pl, sc, dout, x, w, dx, dw, scratch, s);
    if (frozen) {
        rc = frozen_stats(mean, var, d.eps, d.C_out, scratch + sc.stats, s);
        if (rc) return rc;
        stats = scratch + sc.stats;
    }
    // 1. dgamma / dbeta
    const float* s12;
    rc = bn_param_grads(dout, z, stats, scratch + sc.part, scratch + sc.s12, dgamma, dbeta, pl.n_tiles, pl.P, d.C_out, s, &s12);
    if (rc) return rc;
    // 2. dz [P][C_out], written once for the two kernels that read it (frozen: dout gamma rstd, which reads neither z nor the pair)
    const int64_t total4 = (int64_t)pl.P * d.C_out / 4;
    float* const dz = scratch + sc.dz;
    if (frozen) {
        hipLaunchKernelGGL(tnet_dz_kernel<false>, grid1d(total4, 4096), dim3(256), 0, s, dout, (const float*)nullptr, stats, gamma,
                           (const float*)nullptr, dz, total4, d.C_out, pl.P);
        TNET_LAUNCH_CHECK("conv frozen bwd dz")
    } else {
        hipLaunchKernelGGL(tnet_dz_kernel<true>, grid1d(total4, 4096), dim3(256), 0, s, dout, z, stats, gamma, s12, dz, total4, d.C_out, pl.P);
        TNET_LAUNCH_CHECK("conv bwd dz")
    }
    return conv_bwd_products(d, pl, sc, dz, x, w, dx, dw, scratch, s);
}

}  // namespace

extern "C" int64_t ghn3_conv_scratch_floats(const ghn3_conv_desc* g, int backward) { return conv_scratch_floats(g, false, backward); }

extern "C" int ghn3_conv_bn_fwd(const ghn3_conv_desc* g, const float* x, const float* w, const float* gamma, const float* beta, float* z,
                                float* out, float* stats, float* scratch, void* stream_) {
    CDesc d;
    int rc = check_cdesc(g, d);
    if (rc) return rc;
    const bool no_norm = (g->relu & GHN3_CONV_NO_NORM) != 0;       // z is the result: no statistics, no affine map
    if (!x || !w || !z || !scratch || (!no_norm && (!gamma || !beta || !out || !stats))) {
        ghn3_set_error("conv fwd: null pointer");
        return GHN3_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream_;
    const CPlan pl = make_cplan(d);
    const CScratch sc = conv_scratch(d, pl, false, false);
    rc = conv_fwd_launch<EPI_STATS>(d, pl, sc, x, w, z, ConvEpi{}, scratch, s, "conv fwd");
    if (rc || no_norm) return rc;
    return bn_apply_launch(scratch + sc.part, pl.n_tiles, pl.P, d.C_out, d.eps, z, gamma, beta, stats, out, s);
}

extern "C" int ghn3_conv_bn_bwd(const ghn3_conv_desc* g, const float* dout, const float* x, const float* z, const float* stats,
                                const float* w, const float* gamma, float* dx, float* dw, float* dgamma, float* dbeta, float* scratch,
                                void* stream_) {
    return conv_bwd_core(g, false, "conv bwd", dout && x && w && dx && dw && scratch, z && stats && gamma && dgamma && dbeta, dout, x, z, stats,
                         w, gamma, nullptr, nullptr, dx, dw, dgamma, dbeta, scratch, stream_);
}

// ---- the same family behind a norm layer with FROZEN statistics (a BatchNorm in eval mode; see ghn3_dwpw_frozen_fwd) ------------
// Forward: weight pack + the convolution kernel with the affine map in its epilogue (FROZEN), z stored beside out only when the
// caller wants a backward.  Backward: (mean, var) -> (mean, rstd), dgamma / dbeta as with batch statistics, dz = dout gamma rstd
// written once (tnet_dz_kernel<false>: the two kernels that read it take a plain buffer), then dx and dW unchanged.
// Scratch: forward = the weight pack; backward = that of ghn3_conv_bn_bwd followed by the (mean, rstd) pair.
extern "C" int64_t ghn3_conv_frozen_scratch_floats(const ghn3_conv_desc* g, int backward) { return conv_scratch_floats(g, true, backward); }

extern "C" int ghn3_conv_frozen_fwd(const ghn3_conv_desc* g, const float* x, const float* w, const float* gamma, const float* beta,
                                    const float* mean, const float* var, float* z, float* out, float* scratch, void* stream_) {
    CDesc d;
    int rc = check_cdesc(g, d);
    if (rc) return rc;
    if (g->relu & GHN3_CONV_NO_NORM) { ghn3_set_error("conv frozen: GHN3_CONV_NO_NORM has no meaning here"); return GHN3_E_ARG; }
    if (!x || !w || !gamma || !beta || !mean || !var || !out || !scratch) { ghn3_set_error("conv frozen fwd: null pointer"); return GHN3_E_ARG; }
    const CPlan pl = make_cplan(d);
    return conv_fwd_launch<EPI_FROZEN>(d, pl, conv_scratch(d, pl, true, false), x, w, z,
                                       ConvEpi{Frozen{gamma, beta, mean, var, out}, nullptr, nullptr, 0}, scratch, (hipStream_t)stream_,
                                       "conv frozen fwd");
}

extern "C" int ghn3_conv_frozen_bwd(const ghn3_conv_desc* g, const float* dout, const float* x, const float* z, const float* w,
                                    const float* gamma, const float* mean, const float* var, float* dx, float* dw, float* dgamma,
                                    float* dbeta, float* scratch, void* stream_) {
    return conv_bwd_core(g, true, "conv frozen bwd", dout && x && w && dx && dw && scratch, z && gamma && mean && var && dgamma && dbeta, dout,
                         x, z, nullptr, w, gamma, mean, var, dx, dw, dgamma, dbeta, scratch, stream_);
}

// ---- the "act" member: [ReLU ->] convolution -> BatchNorm [-> + skip] -> ReLU, the layer order of ResNet-shaped networks --------
//   out = relu((z - mean) rstd gamma + beta [+ res]),  z = conv(relu(x) if desc->relu else x, w)
// Forward, batch statistics: the launches of ghn3_conv_bn_fwd with tnet_bn_act_apply_kernel as the last one (4: weight pack,
// convolution + per-tile statistics, finalize, apply).  Frozen statistics: the convolution ALONE (the kernel of the batch member:
// its frozen epilogue knows neither skip nor clamp and is not touched), (mean, var) -> (mean, rstd), then the same apply kernel
// (4).  Backward: g = dout 1[out > 0] is never materialised -- the mask is applied where dout is first read, in the per-tile
// partial sums (tnet_bn_act_bwd_partial_kernel) and in the pass that writes dz (tnet_dz_act_kernel), which writes dres = g as
// well --, then conv_bwd_products as for every member: the launches of ghn3_conv_bn_bwd / ghn3_conv_frozen_bwd, none more.
// Saved between the directions: x, z, out (the next layer's input), stats.
// Scratch (ghn3_conv_act_scratch_floats, mode = backward | 2 frozen): the layouts of the members without the ReLU, except the frozen
// forward = the batch member's forward layout (the convolution leaves its per-tile statistics there; they are not read) followed
// by the (mean, rstd) pair.
namespace {

struct ActScratch { CScratch sc; int64_t total; };

ActScratch conv_act_scratch(const CDesc& d, const CPlan& pl, bool frozen, bool backward) {
    ActScratch a;
    a.sc = conv_scratch(d, pl, frozen && backward, backward);
    a.total = a.sc.total;
    if (frozen && !backward) { a.sc.stats = a.total; a.total += 2 * d.C_out; }
    return a;
}

int check_act_desc(const ghn3_conv_desc* g, CDesc& d, const char* who) {
    const int rc = check_cdesc(g, d);
    if (rc) return rc;
    if (g->relu & GHN3_CONV_NO_NORM) { ghn3_set_error("%s: GHN3_CONV_NO_NORM has no meaning here", who); return GHN3_E_ARG; }
    return GHN3_OK;
}

// the last launch of both forwards
int act_apply_launch(const CPlan& pl, int C, const float* z, const float* stats, const float* gamma, const float* beta, const float* res,
                     float* out, hipStream_t s) {
    const int64_t total4 = (int64_t)pl.P * C / 4;
    hipLaunchKernelGGL(tnet_bn_act_apply_kernel, grid1d(total4, ACT_GRID_CAP), dim3(256), 0, s, z, stats, gamma, beta, res, out, total4, C);
    TNET_LAUNCH_CHECK("bn act apply")
    return GHN3_OK;
}

// The backward of both: `stats` = (mean, rstd) of the batch, or null with the frozen (mean, var) given.
int conv_act_bwd_core(const ghn3_conv_desc* g, bool frozen, const char* who, bool required, const float* dout, const float* out,
                      const float* x, const float* z, const float* stats, const float* w, const float* gamma, const float* mean,
                      const float* var, float* dx, float* dw, float* dgamma, float* dbeta, float* dres, float* scratch, void* stream_) {
    CDesc d;
    int rc = check_act_desc(g, d, who);
    if (rc) return rc;
    if (!required) { ghn3_set_error("%s: null pointer", who); return GHN3_E_ARG; }
    hipStream_t s = (hipStream_t)stream_;
    const CPlan pl = make_cplan(d);
    const CScratch sc = conv_act_scratch(d, pl, frozen, true).sc;
    if (frozen) {
        rc = frozen_stats(mean, var, d.eps, d.C_out, scratch + sc.stats, s);
        if (rc) return rc;
        stats = scratch + sc.stats;
    }
    // 1. dgamma / dbeta from the masked gradient
    const float* s12;
    rc = bn_param_grads(dout, z, stats, scratch + sc.part, scratch + sc.s12, dgamma, dbeta, pl.n_tiles, pl.P, d.C_out, s, &s12, out);
    if (rc) return rc;
    // 2. dz [P][C_out] (and dres) from the masked gradient, written once
    const int64_t total4 = (int64_t)pl.P * d.C_out / 4;
    float* const dz = scratch + sc.dz;
    if (frozen) {
        hipLaunchKernelGGL(tnet_dz_act_kernel<false>, grid1d(total4, ACT_GRID_CAP), dim3(256), 0, s, dout, out, (const float*)nullptr, stats,
                           gamma, (const float*)nullptr, dz, dres, total4, d.C_out, pl.P);
    } else {
        hipLaunchKernelGGL(tnet_dz_act_kernel<true>, grid1d(total4, ACT_GRID_CAP), dim3(256), 0, s, dout, out, z, stats, gamma, s12, dz, dres,
                           total4, d.C_out, pl.P);
    }
    TNET_LAUNCH_CHECK("conv act bwd dz")
    return conv_bwd_products(d, pl, sc, dz, x, w, dx, dw, scratch, s);
}

}  // namespace

extern "C" int64_t ghn3_conv_act_scratch_floats(const ghn3_conv_desc* g, int mode) {
    CDesc d;
    const int rc = check_act_desc(g, d, "conv act");
    if (rc) return rc;                                            // GHN3_E_ARG / GHN3_E_LIMIT
    return conv_act_scratch(d, make_cplan(d), (mode & 2) != 0, (mode & 1) != 0).total;
}

extern "C" int ghn3_conv_bn_act_fwd(const ghn3_conv_desc* g, const float* x, const float* w, const float* gamma, const float* beta,
                                    const float* res, float* z, float* out, float* stats, float* scratch, void* stream_) {
    CDesc d;
    int rc = check_act_desc(g, d, "conv act fwd");
    if (rc) return rc;
    if (!x || !w || !gamma || !beta || !z || !out || !stats || !scratch) { ghn3_set_error("conv act fwd: null pointer"); return GHN3_E_ARG; }
    hipStream_t s = (hipStream_t)stream_;
    const CPlan pl = make_cplan(d);
    const CScratch sc = conv_act_scratch(d, pl, false, false).sc;
    rc = conv_fwd_launch<EPI_STATS>(d, pl, sc, x, w, z, ConvEpi{}, scratch, s, "conv act fwd");
    if (rc) return rc;
    hipLaunchKernelGGL(tnet_bn_finalize_kernel, dim3((d.C_out + 15) / 16), dim3(256), 0, s, scratch + sc.part, pl.n_tiles, pl.P, d.C_out, d.eps,
                       stats);
    TNET_LAUNCH_CHECK("bn finalize")
    return act_apply_launch(pl, d.C_out, z, stats, gamma, beta, res, out, s);
}

extern "C" int ghn3_conv_bn_act_bwd(const ghn3_conv_desc* g, const float* dout, const float* out, const float* x, const float* z,
                                    const float* stats, const float* w, const float* gamma, float* dx, float* dw, float* dgamma,
                                    float* dbeta, float* dres, float* scratch, void* stream_) {
    return conv_act_bwd_core(g, false, "conv act bwd", dout && out && x && z && stats && w && gamma && dx && dw && dgamma && dbeta && scratch,
                             dout, out, x, z, stats, w, gamma, nullptr, nullptr, dx, dw, dgamma, dbeta, dres, scratch, stream_);
}

extern "C" int ghn3_conv_frozen_act_fwd(const ghn3_conv_desc* g, const float* x, const float* w, const float* gamma, const float* beta,
                                        const float* mean, const float* var, const float* res, float* z, float* out, float* scratch,
                                        void* stream_) {
    CDesc d;
    int rc = check_act_desc(g, d, "conv frozen act fwd");
    if (rc) return rc;
    if (!x || !w || !gamma || !beta || !mean || !var || !z || !out || !scratch) {
        ghn3_set_error("conv frozen act fwd: null pointer");
        return GHN3_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream_;
    const CPlan pl = make_cplan(d);
    const CScratch sc = conv_act_scratch(d, pl, true, false).sc;
    rc = conv_fwd_launch<EPI_STATS>(d, pl, sc, x, w, z, ConvEpi{}, scratch, s, "conv frozen act fwd");
    if (rc) return rc;
    rc = frozen_stats(mean, var, d.eps, d.C_out, scratch + sc.stats, s);
    if (rc) return rc;
    return act_apply_launch(pl, d.C_out, z, scratch + sc.stats, gamma, beta, res, out, s);
}

extern "C" int ghn3_conv_frozen_act_bwd(const ghn3_conv_desc* g, const float* dout, const float* out, const float* x, const float* z,
                                        const float* w, const float* gamma, const float* mean, const float* var, float* dx, float* dw,
                                        float* dgamma, float* dbeta, float* dres, float* scratch, void* stream_) {
    return conv_act_bwd_core(g, true, "conv frozen act bwd",
                             dout && out && x && z && w && gamma && mean && var && dx && dw && dgamma && dbeta && scratch, dout, out, x, z,
                             nullptr, w, gamma, mean, var, dx, dw, dgamma, dbeta, dres, scratch, stream_);
}

// ---- the "bias" member: [ReLU ->] convolution + bias [+ skip] [-> ReLU], the layers of networks WITHOUT norm layers ------------
//   out = act(conv(relu(x) if desc->relu & 1 else x, w) + bias[c] [+ res]),  act = ReLU with GHN3_CONV_ACT_OUT in desc->relu
// Forward: weight pack + the convolution kernel with the EPI_BIAS epilogue (2 launches); nothing but `out` is stored -- with the
// ReLU it carries the mask 1[out > 0], torch's rule -- and no statistics pass runs.  Backward: ONE pass over dout per 64-pixel
// tile (tnet_bias_bwd_partial_kernel) forms g = dout 1[out > 0] (g = dout without the ReLU), writes it to the scratch's dz (with
// the ReLU) and to dres (when wanted) and leaves the tile's column sums; reduce_rows adds them to dbias in a fixed order; then
// conv_bwd_products on dz -- or on dout itself without the ReLU, which is then never copied: ConvOnly's launches + 2.
// Scratch: forward = the frozen member's forward layout (the weight pack alone); backward = the batch member's backward layout
// (`part` holds the [tiles][C_out] column sums in the first half of its area, s12 is not used).
namespace {

// part[tile][c] = sum over the tile's pixels of g, g = dout 1[out > 0] (out == null: g = dout); dz / dres [P][C] = g where
// non-null.  Geometry, LDS and summation order of tnet_bn_bwd_partial_kernel, in both of its arms, with one sum per channel.
__global__ __launch_bounds__(256) void tnet_bias_bwd_partial_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                                    float* __restrict__ dz, float* __restrict__ dres,
                                                                    float* __restrict__ part, int P, int C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);                               // [ng][C]
    const int nq = C / 4, ng = max(1, 256 / nq);
    const int g = threadIdx.x / nq, q = threadIdx.x % nq, c = 4 * q;
    const int p0 = blockIdx.x * TP, p1 = min(P, p0 + TP);
    auto masked = [&](int64_t at) {
        f32x4 gd = *reinterpret_cast<const f32x4*>(dout + at);
        if (out) gd = act_masked(gd, *reinterpret_cast<const f32x4*>(out + at));
        if (dz) *reinterpret_cast<f32x4*>(dz + at) = gd;
        if (dres) *reinterpret_cast<f32x4*>(dres + at) = gd;
        return gd;
    };
    if (nq > 256) {
        for (int cw = 4 * threadIdx.x; cw < C; cw += 1024) {
            f32x4 s1 = {0.f, 0.f, 0.f, 0.f};
            for (int p = p0; p < p1; ++p) s1 += masked((int64_t)p * C + cw);
            *reinterpret_cast<f32x4*>(part + (int64_t)blockIdx.x * C + cw) = s1;
        }
        return;
    }
    if (g < ng) {
        f32x4 s1 = {0.f, 0.f, 0.f, 0.f};
        for (int p = p0 + g; p < p1; p += ng) s1 += masked((int64_t)p * C + c);
        *reinterpret_cast<f32x4*>(red + g * C + c) = s1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256) {
        float s = 0.f;
        for (int k = 0; k < ng; ++k) s += red[k * C + i];
        part[(int64_t)blockIdx.x * C + i] = s;
    }
}

// bit 1 of desc->relu is the ReLU on x (CDesc.relu, which the kernels test for truth), GHN3_CONV_ACT_OUT the one on the result
int check_bias_desc(const ghn3_conv_desc* g, CDesc& d, const char* who) {
    const int rc = check_cdesc(g, d);
    if (rc) return rc;
    if (g->relu & GHN3_CONV_NO_NORM) { ghn3_set_error("%s: GHN3_CONV_NO_NORM has no meaning here", who); return GHN3_E_ARG; }
    return GHN3_OK;
}

}  // namespace

extern "C" int64_t ghn3_conv_bias_act_scratch_floats(const ghn3_conv_desc* g, int backward) {
    CDesc d;
    const int rc = check_bias_desc(g, d, "conv bias act");
    if (rc) return rc;                                            // GHN3_E_ARG / GHN3_E_LIMIT
    return conv_scratch(d, make_cplan(d), backward == 0, backward != 0).total;
}

extern "C" int ghn3_conv_bias_act_fwd(const ghn3_conv_desc* g, const float* x, const float* w, const float* bias, const float* res,
                                      float* out, float* scratch, void* stream_) {
    CDesc d;
    const int rc = check_bias_desc(g, d, "conv bias act fwd");
    if (rc) return rc;
    if (!x || !w || !bias || !out || !scratch) { ghn3_set_error("conv bias act fwd: null pointer"); return GHN3_E_ARG; }
    const CPlan pl = make_cplan(d);
    const ConvEpi ep = {Frozen{nullptr, nullptr, nullptr, nullptr, out}, bias, res, (g->relu & GHN3_CONV_ACT_OUT) != 0};
    return conv_fwd_launch<EPI_BIAS>(d, pl, conv_scratch(d, pl, true, false), x, w, nullptr, ep, scratch, (hipStream_t)stream_,
                                     "conv bias act fwd");
}

extern "C" int ghn3_conv_bias_act_bwd(const ghn3_conv_desc* g, const float* dout, const float* out, const float* x, const float* w,
                                      float* dx, float* dw, float* dbias, float* dres, float* scratch, void* stream_) {
    CDesc d;
    int rc = check_bias_desc(g, d, "conv bias act bwd");
    if (rc) return rc;
    const bool act = (g->relu & GHN3_CONV_ACT_OUT) != 0;
    if (!dout || (act && !out) || !x || !w || !dx || !dw || !dbias || !scratch) {
        ghn3_set_error("conv bias act bwd: null pointer");
        return GHN3_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream_;
    const CPlan pl = make_cplan(d);
    const CScratch sc = conv_scratch(d, pl, false, true);
    // 1. g = dout 1[out > 0] -> dz (only with the ReLU: without it dout IS dz), dres; the tiles' column sums -> dbias
    float* const dz = act ? scratch + sc.dz : nullptr;
    float* const part = scratch + sc.part;
    const int nq = d.C_out / 4, ng = std::max(1, 256 / nq);
    hipLaunchKernelGGL(tnet_bias_bwd_partial_kernel, dim3(pl.n_tiles), dim3(256), nq > 256 ? 0 : (size_t)ng * d.C_out * 4, s, dout,
                       act ? out : nullptr, dz, dres, part, pl.P, d.C_out);
    TNET_LAUNCH_CHECK("conv bias bwd partial")
    rc = reduce_rows(part, pl.n_tiles, d.C_out, dbias, 0, 0, s, "conv bias bwd reduce");
    if (rc) return rc;
    // 2. weight pack, dx, dW and its reduction, as for every member
    return conv_bwd_products(d, pl, sc, act ? dz : dout, x, w, dx, dw, scratch, s);
}

// ---------------------------------------------------------------------------------------------------------------------
// squeeze-and-excitation with a hard-swish gate (round 6; ChannelSELayer, ops.py:239-274):
//   s = mean_hw(x);  h = relu(W1 s + b1);  a = W2 h + b2;  y = x * hardswish(a)
// One workgroup per sample: the reference runs mean, two hipBLASLt GEMMs of a 64-row batch (80 us of host dispatch each),
// ReLU, hard-swish and the product as ~8 launches forward and ~14 backward; here 1 and 2.  NHWC activations as the other ops.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ float hswish(float a) { return a * fminf(fmaxf(a + 3.f, 0.f), 6.f) * (1.f / 6.f); }
// (torch's hardswish_backward: 0 below -3, x / 3 + 0.5 up to 3, 1 above)
__device__ __forceinline__ float hswish_grad(float a) { return a < -3.f ? 0.f : (a <= 3.f ? a * (1.f / 3.f) + 0.5f : 1.f); }

// v[c] = sum over the sample's pixels of a[p][c] (* b[p][c] when b != nullptr), c = 0 .. C - 1, into LDS `out` (floats);
// `red` = 256 float4 of LDS.  Threads = channel quad x pixel lane.
__device__ __forceinline__ void se_pixel_sum(const float* __restrict__ a, const float* __restrict__ b, int HW, int C, f32x4* red,
                                             float* out, float scale) {
    const int nq = C / 4, PL = max(1, 256 / nq), cq = threadIdx.x % nq, pl = threadIdx.x / nq;
    if (nq > 256) {
        // more quads than threads (C > 1024): a thread takes the quads tid, tid + 256, ... over the pixels in sequence; `red` unused
        for (int q = threadIdx.x; q < nq; q += 256) {
            f32x4 sum = {0.f, 0.f, 0.f, 0.f};
            for (int p = 0; p < HW; ++p) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(a + (int64_t)p * C + 4 * q);
                if (b) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(b + (int64_t)p * C + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) sum[e] = fmaf(u[e], v[e], sum[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) sum[e] += u[e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) out[4 * q + e] = sum[e] * scale;
        }
        __syncthreads();
        return;
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (pl < PL) {
        for (int p = pl; p < HW; p += PL) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(a + (int64_t)p * C + 4 * cq);
            if (b) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(b + (int64_t)p * C + 4 * cq);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(u[e], v[e], acc[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += u[e];
            }
        }
        red[pl * nq + cq] = acc;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nq; q += 256) {
        f32x4 sum = red[q];
        for (int l = 1; l < PL; ++l) {
            const f32x4 v = red[l * nq + q];
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[e] += v[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) out[4 * q + e] = sum[e] * scale;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void tnet_se_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w1,
                                                          const float* __restrict__ b1, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, float* __restrict__ y, float* __restrict__ save,
                                                          const int HW, const int C, const int J) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f32x4* red = reinterpret_cast<f32x4*>(smem);                               // [256]
    float* s = reinterpret_cast<float*>(smem + 4096);                          // [C]
    float* g = s + C;                                                          // [C]
    float* h = g + C;                                                          // [J]
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* xn = x + (int64_t)n * HW * C;
    float* sv = save + (int64_t)n * (2 * C + J);
    se_pixel_sum(xn, nullptr, HW, C, red, s, 1.f / (float)HW);
    for (int j = wv; j < J; j += 4) {                                          // h = relu(W1 s + b1): a wave per output
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc = fmaf(w1[(int64_t)j * C + c], s[c], acc);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if (lane == 0) h[j] = fmaxf(acc + b1[j], 0.f);
    }
    __syncthreads();
    for (int c = wv; c < C; c += 4) {                                          // a = W2 h + b2, g = hardswish(a)
        float acc = 0.f;
        for (int j = lane; j < J; j += 64) acc = fmaf(w2[(int64_t)c * J + j], h[j], acc);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if (lane == 0) {
            const float a = acc + b2[c];
            g[c] = hswish(a);
            sv[C + c] = a;
        }
    }
    for (int c = tid; c < C; c += 256) sv[c] = s[c];
    for (int j = tid; j < J; j += 256) sv[2 * C + j] = h[j];
    __syncthreads();
    const int nq = C / 4;
    float* yn = y + (int64_t)n * HW * C;
    for (int i = tid; i < HW * nq; i += 256) {
        const int c4 = (i % nq) * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(xn + 4 * (int64_t)i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= g[c4 + e];
        *reinterpret_cast<f32x4*>(yn + 4 * (int64_t)i) = v;
    }
}

// per sample: dx, and the vectors the parameter gradients are sums of: vec[n] = [da (C) | dz1 (J)]
__global__ __launch_bounds__(256) void tnet_se_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ w1, const float* __restrict__ w2,
                                                          const float* __restrict__ save, float* __restrict__ dx, float* __restrict__ vec,
                                                          const int HW, const int C, const int J) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    float* da = reinterpret_cast<float*>(smem + 4096);                         // [C]: dg, then da in place
    float* ds = da + C;                                                        // [C]
    float* dz = ds + C;                                                        // [J]
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* xn = x + (int64_t)n * HW * C;
    const float* dyn = dy + (int64_t)n * HW * C;
    const float* sv = save + (int64_t)n * (2 * C + J);
    float* vn = vec + (int64_t)n * (C + J);
    se_pixel_sum(dyn, xn, HW, C, red, da, 1.f);                                // dg[c] = sum_p dy x
    for (int c = tid; c < C; c += 256) {
        const float v = da[c] * hswish_grad(sv[C + c]);
        da[c] = v;
        vn[c] = v;
    }
    __syncthreads();
    for (int j = tid; j < J; j += 256) {                                       // dh = W2^T da, masked by the ReLU
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(w2[(int64_t)c * J + j], da[c], acc);
        const float v = sv[2 * C + j] > 0.f ? acc : 0.f;
        dz[j] = v;
        vn[C + j] = v;
    }
    __syncthreads();
    const float inv = 1.f / (float)HW;
    for (int c = tid; c < C; c += 256) {                                       // ds = W1^T dz1, spread over the pixels
        float acc = 0.f;
        for (int j = 0; j < J; ++j) acc = fmaf(w1[(int64_t)j * C + c], dz[j], acc);
        ds[c] = acc * inv;
    }
    __syncthreads();
    const int nq = C / 4;
    float* dxn = dx + (int64_t)n * HW * C;
    for (int i = tid; i < HW * nq; i += 256) {
        const int c4 = (i % nq) * 4;
        const f32x4 gy = *reinterpret_cast<const f32x4*>(dyn + 4 * (int64_t)i);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(gy[e], hswish(sv[C + c4 + e]), ds[c4 + e]);
        *reinterpret_cast<f32x4*>(dxn + 4 * (int64_t)i) = v;
    }
}

// dW2[c][j] = sum_n da[n][c] h[n][j];  dW1[j][c] = sum_n dz1[n][j] s[n][c];  db2 = sum_n da;  db1 = sum_n dz1  (fixed order over n)
__global__ __launch_bounds__(256) void tnet_se_wgrad_kernel(const float* __restrict__ vec, const float* __restrict__ save,
                                                            float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                            float* __restrict__ db2, const int N, const int C, const int J) {
    const int64_t cj = (int64_t)C * J, total = 2 * cj + C + J;
    const int sv_ld = 2 * C + J, v_ld = C + J;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        float acc = 0.f;
        if (i < cj) {                                                          // dW2[c][j]
            const int c = (int)(i / J), j = (int)(i % J);
            for (int n = 0; n < N; ++n) acc = fmaf(vec[(int64_t)n * v_ld + c], save[(int64_t)n * sv_ld + 2 * C + j], acc);
            dw2[i] = acc;
        } else if (i < 2 * cj) {                                               // dW1[j][c]
            const int64_t r = i - cj;
            const int j = (int)(r / C), c = (int)(r % C);
            for (int n = 0; n < N; ++n) acc = fmaf(vec[(int64_t)n * v_ld + C + j], save[(int64_t)n * sv_ld + c], acc);
            dw1[r] = acc;
        } else if (i < 2 * cj + C) {
            const int c = (int)(i - 2 * cj);
            for (int n = 0; n < N; ++n) acc += vec[(int64_t)n * v_ld + c];
            db2[c] = acc;
        } else {
            const int j = (int)(i - 2 * cj - C);
            for (int n = 0; n < N; ++n) acc += vec[(int64_t)n * v_ld + C + j];
            db1[j] = acc;
        }
    }
}

int check_se(int N, int HW, int C, int J) {
    if (N <= 0 || HW <= 0 || C <= 0 || J <= 0) { ghn3_set_error("se: non-positive size"); return GHN3_E_ARG; }
    if ((C & 3) || C > 4096 || J > 4096 || (int64_t)N * HW * C >= ((int64_t)1 << 31)) {
        ghn3_set_error("se: needs C a multiple of 4, C, J <= 4096 and fewer than 2^31 activations (got C = %d, J = %d)", C, J);
        return GHN3_E_LIMIT;
    }
    return GHN3_OK;
}

}  // namespace

extern "C" int ghn3_se_fwd(int N, int HW, int C, int J, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                           float* y, float* save, void* stream_) {
    int rc = check_se(N, HW, C, J);
    if (rc) return rc;
    if (!x || !w1 || !b1 || !w2 || !b2 || !y || !save) { ghn3_set_error("se fwd: null pointer"); return GHN3_E_ARG; }
    const size_t lds = (size_t)4096 + (size_t)(2 * C + J) * 4;    // (52 KB at the widest layer)
    rc = tnet_raise_lds(tnet_se_fwd_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(tnet_se_fwd_kernel, dim3(N), dim3(256), lds, (hipStream_t)stream_, x, w1, b1, w2, b2, y, save, HW, C, J);
    TNET_LAUNCH_CHECK("se fwd")
    return GHN3_OK;
}

extern "C" int ghn3_se_bwd(int N, int HW, int C, int J, const float* dy, const float* x, const float* w1, const float* w2, const float* save,
                           float* dx, float* dw1, float* db1, float* dw2, float* db2, float* scratch, void* stream_) {
    int rc = check_se(N, HW, C, J);
    if (rc) return rc;
    if (!dy || !x || !w1 || !w2 || !save || !dx || !dw1 || !db1 || !dw2 || !db2 || !scratch) {
        ghn3_set_error("se bwd: null pointer");
        return GHN3_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream_;
    const size_t lds = (size_t)4096 + (size_t)(2 * C + J) * 4;
    rc = tnet_raise_lds(tnet_se_bwd_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(tnet_se_bwd_kernel, dim3(N), dim3(256), lds, s, dy, x, w1, w2, save, dx, scratch, HW, C, J);
    TNET_LAUNCH_CHECK("se bwd")
    const int64_t total = (int64_t)2 * C * J + C + J;
    hipLaunchKernelGGL(tnet_se_wgrad_kernel, dim3((int)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, scratch, save, dw1, db1, dw2,
                       db2, N, C, J);
    TNET_LAUNCH_CHECK("se wgrad")
    return GHN3_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// k x k max / average pooling on NHWC activations (round 6; the `max_pool_3x3` / `avg_pool_3x3` ops of ops.py:289-291 and the
// stems' MaxPool2d(3, 2, 1)): ATen's pooling kernels return wrong input gradients for channels_last tensors on this ROCm build, so
// every pooling layer behind a fused layer paid two layout copies.  Average pooling counts valid taps only
// (count_include_pad = False, as the search space builds it); max pooling keeps the FIRST maximum in (kh, kw) scan order as
// torch does and stores its tap in one byte per output element.  Backward as a gather per input pixel: no atomics.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct PDesc { int N, H, W, C, k, stride, pad, Ho, Wo, mode; };

__global__ __launch_bounds__(256) void tnet_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            unsigned char* __restrict__ idx, const PDesc d, const int64_t total) {
    const int nq = d.C / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int cq = (int)(i % nq);
        const int64_t p = i / nq;
        const int ow = (int)(p % d.Wo), oh = (int)((p / d.Wo) % d.Ho), n = (int)(p / ((int64_t)d.Wo * d.Ho));
        const int ih0 = oh * d.stride - d.pad, iw0 = ow * d.stride - d.pad;
        f32x4 acc = d.mode ? f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY} : f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned arg[4] = {0, 0, 0, 0};
        int cnt = 0;
        for (int kh = 0; kh < d.k; ++kh) {
            const int ih = ih0 + kh;
            if (ih < 0 || ih >= d.H) continue;
            for (int kw = 0; kw < d.k; ++kw) {
                const int iw = iw0 + kw;
                if (iw < 0 || iw >= d.W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((int64_t)n * d.H + ih) * d.W + iw) * d.C + 4 * cq);
                ++cnt;
                if (d.mode) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (v[e] > acc[e] || v[e] != v[e]) { acc[e] = v[e]; arg[e] = (unsigned)(kh * d.k + kw); }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += v[e];
                }
            }
        }
        if (!d.mode) {
            const float inv = 1.f / (float)max(cnt, 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] *= inv;
        } else {
            *reinterpret_cast<unsigned*>(idx + 4 * i) = arg[0] | (arg[1] << 8) | (arg[2] << 16) | (arg[3] << 24);
        }
        *reinterpret_cast<f32x4*>(y + 4 * i) = acc;
    }
}

__device__ __forceinline__ int pool_count(const PDesc& d, int o, int size) {     // valid taps of output index o along one axis
    const int lo = max(o * d.stride - d.pad, 0), hi = min(o * d.stride - d.pad + d.k, size);
    return max(hi - lo, 0);
}

__global__ __launch_bounds__(256) void tnet_pool_bwd_kernel(const float* __restrict__ dy, const unsigned char* __restrict__ idx,
                                                            float* __restrict__ dx, const PDesc d, const int64_t total) {
    const int nq = d.C / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int cq = (int)(i % nq);
        const int64_t p = i / nq;
        const int iw = (int)(p % d.W), ih = (int)((p / d.W) % d.H), n = (int)(p / ((int64_t)d.W * d.H));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        // outputs whose window holds (ih, iw): oh * stride - pad <= ih < oh * stride - pad + k
        const int oh_lo = max(0, (ih + d.pad - d.k + d.stride) / d.stride), oh_hi = min(d.Ho - 1, (ih + d.pad) / d.stride);
        const int ow_lo = max(0, (iw + d.pad - d.k + d.stride) / d.stride), ow_hi = min(d.Wo - 1, (iw + d.pad) / d.stride);
        for (int oh = oh_lo; oh <= oh_hi; ++oh) {
            const int kh = ih - (oh * d.stride - d.pad);
            if (kh < 0 || kh >= d.k) continue;
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                const int kw = iw - (ow * d.stride - d.pad);
                if (kw < 0 || kw >= d.k) continue;
                const int64_t o = (((int64_t)n * d.Ho + oh) * d.Wo + ow) * nq + cq;
                const f32x4 g = *reinterpret_cast<const f32x4*>(dy + 4 * o);
                if (d.mode) {
                    const unsigned a = *reinterpret_cast<const unsigned*>(idx + 4 * o), t = (unsigned)(kh * d.k + kw);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (((a >> (8 * e)) & 255u) == t) acc[e] += g[e];
                } else {
                    const float inv = 1.f / (float)max(pool_count(d, oh, d.H) * pool_count(d, ow, d.W), 1);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = fmaf(g[e], inv, acc[e]);
                }
            }
        }
        *reinterpret_cast<f32x4*>(dx + 4 * i) = acc;
    }
}

int check_pdesc(const ghn3_pool_desc* g, PDesc& d) {
    if (!g) { ghn3_set_error("pool: null descriptor"); return GHN3_E_ARG; }
    d = PDesc{g->N, g->H, g->W, g->C, g->k, g->stride, g->pad, g->Ho, g->Wo, g->mode};
    if (d.N <= 0 || d.H <= 0 || d.W <= 0 || d.C <= 0 || d.k <= 0 || d.stride <= 0 || d.pad < 0 || (d.mode != 0 && d.mode != 1)) {
        ghn3_set_error("pool: bad descriptor");
        return GHN3_E_ARG;
    }
    if ((d.C & 3) || d.k > 15 || 2 * d.pad > d.k) {
        ghn3_set_error("pool: needs C a multiple of 4, k <= 15, pad <= k / 2 (got C = %d, k = %d, pad = %d)", d.C, d.k, d.pad);
        return GHN3_E_LIMIT;
    }
    const int ho = (d.H + 2 * d.pad - d.k) / d.stride + 1, wo = (d.W + 2 * d.pad - d.k) / d.stride + 1;
    if (ho != d.Ho || wo != d.Wo || ho <= 0 || wo <= 0) {
        ghn3_set_error("pool: output size %d x %d does not match the pooling arithmetic (%d x %d, floor mode)", d.Ho, d.Wo, ho, wo);
        return GHN3_E_ARG;
    }
    if ((int64_t)d.N * d.H * d.W * d.C >= ((int64_t)1 << 31)) { ghn3_set_error("pool: 2^31 activations or more"); return GHN3_E_LIMIT; }
    return GHN3_OK;
}

}  // namespace

extern "C" int ghn3_pool_fwd(const ghn3_pool_desc* g, const float* x, float* y, unsigned char* idx, void* stream_) {
    PDesc d;
    int rc = check_pdesc(g, d);
    if (rc) return rc;
    if (!x || !y || (d.mode == 1 && !idx)) { ghn3_set_error("pool fwd: null pointer"); return GHN3_E_ARG; }
    const int64_t total = (int64_t)d.N * d.Ho * d.Wo * (d.C / 4);
    hipLaunchKernelGGL(tnet_pool_fwd_kernel, dim3((int)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream_, x, y, idx,
                       d, total);
    TNET_LAUNCH_CHECK("pool fwd")
    return GHN3_OK;
}

extern "C" int ghn3_pool_bwd(const ghn3_pool_desc* g, const float* dy, const unsigned char* idx, float* dx, void* stream_) {
    PDesc d;
    int rc = check_pdesc(g, d);
    if (rc) return rc;
    if (!dy || !dx || (d.mode == 1 && !idx)) { ghn3_set_error("pool bwd: null pointer"); return GHN3_E_ARG; }
    const int64_t total = (int64_t)d.N * d.H * d.W * (d.C / 4);
    hipLaunchKernelGGL(tnet_pool_bwd_kernel, dim3((int)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream_, dy, idx,
                       dx, d, total);
    TNET_LAUNCH_CHECK("pool bwd")
    return GHN3_OK;
}
