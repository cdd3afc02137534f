// Target-network layers: the patch embedding of the ImageNet-sized ViT-style networks, `Conv2d(3, C, 16, stride = 16, bias = False)`
// on 224 x 224 images -- in general a bias-free, ungrouped, unpadded convolution whose windows do not overlap (stride >= kernel)
// with a kernel of 8 .. 32 taps a side, which the dense-convolution family (target_ops.hip: kernel <= 7) refuses.  Such a
// convolution is a plain GEMM over a permutation of the image,
//
//     z[p][co] = sum_k xg[p][k] w[co][k],   p = (n, oh, ow),  k = (ci, a, b),  xg[p][k] = x[n, ci, oh sh + a, ow sw + b],
//
// and the weight [C_out][C_in][kh][kw] is already K-contiguous in that reduction order.
//
//   tnet_patch_gemm<NT, DX = false>   forward: a workgroup owns 64 output pixels x 16 NT output columns (the columns are split
//                    over blockIdx.y so that small grids still cover the chip); per 32-wide reduction chunk the pixel rows are
//                    gathered from the image AS STORED (NCHW or NHWC strides, scalar loads: nothing assumes an aligned window row,
//                    the three image channels are read as three) and the weight rows are read in place; both are cut into three
//                    bf16 pieces while staged and multiplied with the six products of mma_terms<3> (fp32-grade, fp32 accumulate);
//                    the loads of chunks i + 1 and i + 2 are in flight during the products of chunk i (two register sets -> the
//                    other LDS stage, one barrier per chunk).  z is written [P][C_out] (NHWC).
//   tnet_patch_gemm<NT, DX = true>    dx = dz . W, same tile and pipeline: rows of dz [P][C_out], reduction over C_out, the weight
//                    staged transposed, the result scattered to the image's own layout.
//   tnet_patch_gaps  zeros the elements of dx no window reaches (stride > kernel, trailing rows / columns): with the scatter every
//                    element of dx is written exactly once.  Not launched when the windows tile the image.
//   tnet_patch_wgrad dw[co][k] = sum_p dz[p][co] xg[p][k] per pixel chunk on v_mfma_f32_16x16x4_f32 (exact fp32 products) as
//                    tnet_wgrad_kernel (tnet_wgrad.hip) with the gather in its X loads: a workgroup per (chunk, 32 x 32 block);
//                    the chunk's product goes to its slot of the partials, which tnet_reduce sums in chunk order into dw -- the
//                    parameter's own order --, or straight to dw when there is one chunk.
//
// No float atomics, nothing allocated or synchronised here.  Limits: ghn3_hip.h (ghn3_patch_fwd).

#include <algorithm>
#include "tnet_common.h"

namespace {

constexpr int TP = 64;       // pixels per tile (4 waves x 16-row MFMA tiles)
constexpr int S = 3;         // bf16 pieces per operand

struct PDesc {
    int N, H, W, C_in, C_out, kh, kw, sh, sw, Ho, Wo, nhwc;
    int K, P;                       // reduction length C_in kh kw, output pixels N Ho Wo
    int64_t sN, sC, sH, sW;         // strides of x (and dx) in floats
};

// offset of the first element of output pixel p's window (channel 0)
__device__ __forceinline__ int64_t pix_base(const PDesc& d, int p) {
    const int hw = d.Ho * d.Wo, n = p / hw, r = p - n * hw, oh = r / d.Wo, ow = r - oh * d.Wo;
    return n * d.sN + (int64_t)(oh * d.sh) * d.sH + (int64_t)(ow * d.sw) * d.sW;
}

// Walks k = (ci, a, b) in the weight's order: `off` = offset of element k inside a window.
struct TapWalk {
    int a, b;
    int64_t off;
    __device__ __forceinline__ TapWalk(const PDesc& d, int k) {
        const int taps = d.kh * d.kw, ci = k / taps, r = k - ci * taps;
        a = r / d.kw; b = r - a * d.kw;
        off = ci * d.sC + a * d.sH + b * d.sW;
    }
    __device__ __forceinline__ void next(const PDesc& d) {
        ++b; off += d.sW;
        if (b == d.kw) {
            b = 0; ++a; off += d.sH - d.kw * d.sW;
            if (a == d.kh) { a = 0; off += d.sC - d.kh * d.sH; }
        }
    }
};

// DX = false: dst = z [P][C_out] from src = x;  DX = true: dst = dx (the image's layout) from src = dz [P][C_out].
template <int NT, bool DX>
__global__ __launch_bounds__(256) void tnet_patch_gemm_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                              float* __restrict__ dst, const PDesc d) {
    constexpr int A_BUF = S * TP * LDK, B_BUF = S * 16 * NT * LDK;             // 16-bit elements per stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned short* As = reinterpret_cast<unsigned short*>(smem);              // [2][S][TP][LDK]
    unsigned short* Bs = As + 2 * A_BUF;                                       // [2][S][16 NT][LDK]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, kc = lane >> 4;
    const int p0 = blockIdx.x * TP, col0 = blockIdx.y * 16 * NT;
    const int R = DX ? d.C_out : d.K, cols = DX ? d.K : d.C_out;               // reduction length, output columns
    const int n_it = (R + KC - 1) / KC;
    const int ai = tid >> 2, ak = (tid & 3) * 8;                               // this thread's A row (pixel) and k offset
    const bool aok = p0 + ai < d.P;
    const int64_t abase = !aok ? 0 : DX ? (int64_t)(p0 + ai) * d.C_out : pix_base(d, p0 + ai);
    // prefetched operands: two register sets, so that the loads of chunks i + 1 and i + 2 are in flight during chunk i
    float av0[8], bv0[2 * NT], av1[8], bv1[2 * NT];
    auto fetch = [&](int it, float (&av)[8], float (&bv)[2 * NT]) {
        const int c0 = it * KC, c = c0 + ak;
#pragma unroll
        for (int e = 0; e < 8; ++e) av[e] = 0.f;
        if (aok && c < R) {
            if (DX) {                                                          // (C_out is a multiple of 4: whole quads)
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + abase + c);
                const f32x4 v1 = c + 4 < R ? *reinterpret_cast<const f32x4*>(src + abase + c + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) { av[e] = v0[e]; av[4 + e] = v1[e]; }
            } else {
                TapWalk t(d, c);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (c + e < R) av[e] = src[abase + t.off];
                    t.next(d);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int i = tid + 256 * u;                                       // a pair of neighbours along the reduction
            float v0 = 0.f, v1 = 0.f;
            if (DX) {                                                          // B[row = k][reduction = co] = w[co][k]
                const int k = col0 + (i & (16 * NT - 1)), co = c0 + 2 * (i / (16 * NT));
                if (k < d.K && co < d.C_out) v0 = w[(int64_t)co * d.K + k];
                if (k < d.K && co + 1 < d.C_out) v1 = w[(int64_t)(co + 1) * d.K + k];
            } else {                                                           // B[row = co][reduction = k] = w[co][k]
                const int co = col0 + (i >> 4), k = c0 + 2 * (i & 15);
                if (co < d.C_out && k < d.K) v0 = w[(int64_t)co * d.K + k];
                if (co < d.C_out && k + 1 < d.K) v1 = w[(int64_t)co * d.K + k + 1];
            }
            bv[2 * u] = v0; bv[2 * u + 1] = v1;
        }
    };
    auto stage = [&](int buf, const float (&av)[8], const float (&bv)[2 * NT]) {   // registers -> LDS stage `buf`, cut into pieces
        unsigned short* A = As + buf * A_BUF;
        unsigned* B = reinterpret_cast<unsigned*>(Bs + buf * B_BUF);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = av[e];
#pragma unroll
        for (int q = 0; q < S; ++q) {
            unsigned h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                h[e] = bf16_pk(v[2 * e], v[2 * e + 1]);
                v[2 * e] -= __uint_as_float(h[e] << 16);
                v[2 * e + 1] -= __uint_as_float(h[e] & 0xffff0000u);
            }
            *reinterpret_cast<uint4*>(A + q * TP * LDK + ai * LDK + ak) = uint4{h[0], h[1], h[2], h[3]};
        }
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int i = tid + 256 * u;
            const int at = DX ? (i & (16 * NT - 1)) * LDK + 2 * (i / (16 * NT)) : (i >> 4) * LDK + 2 * (i & 15);
            float v0 = bv[2 * u], v1 = bv[2 * u + 1];
#pragma unroll
            for (int q = 0; q < S; ++q) {
                const unsigned h = bf16_pk(v0, v1);
                B[(q * 16 * NT * LDK + at) >> 1] = h;
                v0 -= __uint_as_float(h << 16);
                v1 -= __uint_as_float(h & 0xffff0000u);
            }
        }
    };
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto products = [&](int buf) {
        const unsigned short* A = As + buf * A_BUF;
        const unsigned short* B = Bs + buf * B_BUF;
        u16x8 af[S];
#pragma unroll
        for (int q = 0; q < S; ++q) af[q] = frag(A + q * TP * LDK, 16 * wv + r16, kc);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            u16x8 bf[S];
#pragma unroll
            for (int q = 0; q < S; ++q) bf[q] = frag(B + q * 16 * NT * LDK, 16 * j + r16, kc);
            acc[j] = mma_terms<S>(af, bf, acc[j]);
        }
    };
    // chunk i is multiplied from LDS stage i & 1 while chunk i + 1 waits in one register set to be staged behind the products
    // and chunk i + 2 is being loaded into the other: one barrier per chunk
    fetch(0, av0, bv0);
    stage(0, av0, bv0);
    if (n_it > 1) fetch(1, av1, bv1);
    __syncthreads();
    for (int it = 0; it < n_it; it += 2) {
        if (it + 2 < n_it) fetch(it + 2, av0, bv0);
        products(0);
        if (it + 1 < n_it) stage(1, av1, bv1);
        __syncthreads();
        if (it + 1 >= n_it) break;
        if (it + 3 < n_it) fetch(it + 3, av1, bv1);
        products(1);
        if (it + 2 < n_it) stage(0, av0, bv0);
        __syncthreads();
    }
    // C/D: row (pixel) 16 wv + r16, columns 16 j + 4 kc + e
    const int prow = p0 + 16 * wv + r16;
    if (prow >= d.P) return;
    if (DX) {
        const int64_t pbase = pix_base(d, prow);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int k = col0 + 16 * j + 4 * kc;
            if (k >= d.K) continue;
            TapWalk t(d, k);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (k + e < d.K) dst[pbase + t.off] = acc[j][e];
                t.next(d);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = col0 + 16 * j + 4 * kc;
            if (col < cols) *reinterpret_cast<f32x4*>(dst + (int64_t)prow * d.C_out + col) = acc[j];
        }
    }
}

// dx = 0 wherever no window reaches: one thread per element of the image, in storage order
__global__ __launch_bounds__(256) void tnet_patch_gaps_kernel(float* __restrict__ dx, const PDesc d, const int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t px = d.nhwc ? i / d.C_in : i;                            // ((n [c]) H + h) W + w
        const int wq = (int)(px % d.W), h = (int)((px / d.W) % d.H);
        const bool covered = h / d.sh < d.Ho && h % d.sh < d.kh && wq / d.sw < d.Wo && wq % d.sw < d.kw;
        if (!covered) dx[i] = 0.f;
    }
}

// out[chunk][co][k] = sum over the chunk's pixels of dz[p][co] xg[p][k]; workgroup = (chunk, 32 co x 32 k), a wave per 16 x 16
// quarter (tnet_wgrad_kernel's product with the window gather in its X loads); out = dw itself when there is one chunk
__global__ __launch_bounds__(256) void tnet_patch_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                               float* __restrict__ out, const PDesc d, const int chunks,
                                                               const int chunk_px, const int tiles_n) {
    const int chunk = blockIdx.x % chunks, tile = blockIdx.x / chunks;
    const int tn = tile % tiles_n, tk = tile / tiles_n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int n0 = tn * 32 + (wave & 1) * 16, k0 = tk * 32 + (wave >> 1) * 16;
    const int n = n0 + i, k = k0 + i;
    const bool nok = n < d.C_out, kok = k < d.K;
    const int64_t koff = kok ? TapWalk(d, k).off : 0;
    const int rb = chunk * chunk_px, re = min(rb + chunk_px, d.P), hw = d.Ho * d.Wo;
    const int nc = nok ? n : 0;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    // (64 rows a step, every load unconditional on a clamped address: the 32 loads of a step are issued together and a wave
    // waits for memory once per 64 rows; rows beyond the chunk contribute zeros)
    for (int r0 = rb; r0 < re; r0 += 64) {
        float a[4][4], b[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int r = r0 + 16 * s + 4 * q;
            int pn = r / hw, oh = (r - pn * hw) / d.Wo, ow = r - pn * hw - oh * d.Wo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool rin = r + j < d.P, rok = r + j < re;
                const float gv = dz[rin ? (int64_t)(r + j) * d.C_out + nc : 0];
                const float xv = x[rin ? pn * d.sN + (int64_t)(oh * d.sh) * d.sH + (int64_t)(ow * d.sw) * d.sW + koff : 0];
                a[s][j] = (rok && nok) ? gv : 0.f;
                b[s][j] = (rok && kok) ? xv : 0.f;
                if (++ow == d.Wo) { ow = 0; if (++oh == d.Ho) { oh = 0; ++pn; } }
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][j], b[s][j], acc, 0, 0, 0);
    }
    // C/D: row (co) 4 q + g, col (k) i
    if (kok) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int nn = n0 + 4 * q + g;
            if (nn < d.C_out) out[((int64_t)chunk * d.C_out + nn) * d.K + k] = acc[g];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PATCH_MIN_K = 8, PATCH_MAX_K = 32, PATCH_MAX_IN = 4, PATCH_MAX_OUT = 4096, PATCH_MAX_RED = 4096;

int check_pdesc(const ghn3_patch_desc* g, PDesc& d) {
    if (!g) { ghn3_set_error("patch: null descriptor"); return GHN3_E_ARG; }
    d = PDesc{g->N, g->H, g->W, g->C_in, g->C_out, g->kh, g->kw, g->stride_h, g->stride_w, g->Ho, g->Wo, g->nhwc, 0, 0, 0, 0, 0, 0};
    if (d.N <= 0 || d.H <= 0 || d.W <= 0 || d.C_in <= 0 || d.C_out <= 0 || d.kh <= 0 || d.kw <= 0 || d.sh <= 0 || d.sw <= 0 ||
        (d.nhwc != 0 && d.nhwc != 1)) {
        ghn3_set_error("patch: non-positive size or unknown layout in the descriptor");
        return GHN3_E_ARG;
    }
    const int kmax = std::max(d.kh, d.kw);
    if (kmax < PATCH_MIN_K || kmax > PATCH_MAX_K || d.C_in > PATCH_MAX_IN || (int64_t)d.C_in * d.kh * d.kw > PATCH_MAX_RED ||
        (d.C_out & 3) || d.C_out > PATCH_MAX_OUT || d.sh < d.kh || d.sw < d.kw) {
        ghn3_set_error("patch: needs max(kh, kw) in %d .. %d, C_in <= %d, C_in kh kw <= %d, C_out a multiple of 4 and <= %d, "
                       "stride >= kernel (got %d -> %d, %d x %d, stride %d x %d)", PATCH_MIN_K, PATCH_MAX_K, PATCH_MAX_IN,
                       PATCH_MAX_RED, PATCH_MAX_OUT, d.C_in, d.C_out, d.kh, d.kw, d.sh, d.sw);
        return GHN3_E_LIMIT;
    }
    const int ho = d.H < d.kh ? 0 : (d.H - d.kh) / d.sh + 1, wo = d.W < d.kw ? 0 : (d.W - d.kw) / d.sw + 1;
    if (ho != d.Ho || wo != d.Wo || ho <= 0 || wo <= 0) {
        ghn3_set_error("patch: output size %d x %d does not match the convolution arithmetic (%d x %d)", d.Ho, d.Wo, ho, wo);
        return GHN3_E_ARG;
    }
    if ((int64_t)d.N * d.H * d.W * d.C_in >= ((int64_t)1 << 31) || (int64_t)d.N * d.Ho * d.Wo * d.C_out >= ((int64_t)1 << 31)) {
        ghn3_set_error("patch: tensors of 2^31 elements or more are not supported");
        return GHN3_E_LIMIT;
    }
    d.K = d.C_in * d.kh * d.kw;
    d.P = d.N * d.Ho * d.Wo;
    if (d.nhwc) { d.sC = 1; d.sW = d.C_in; d.sH = (int64_t)d.W * d.C_in; }
    else { d.sW = 1; d.sH = d.W; d.sC = (int64_t)d.H * d.W; }
    d.sN = (int64_t)d.C_in * d.H * d.W;
    return GHN3_OK;
}

// The weight gradient's pixel chunks: enough (chunk, block) workgroups to cover the chip, at least 64 pixels a chunk.
struct PPlan { int tiles_n, tiles, chunks, chunk_px; };

PPlan make_pplan(const PDesc& d) {
    PPlan pl;
    pl.tiles_n = (d.C_out + 31) / 32;
    pl.tiles = pl.tiles_n * ((d.K + 31) / 32);
    const int want = std::max(1, std::min((1024 + pl.tiles - 1) / pl.tiles, (d.P + 63) / 64));
    pl.chunk_px = ((d.P + want - 1) / want + 15) / 16 * 16;
    pl.chunks = (d.P + pl.chunk_px - 1) / pl.chunk_px;
    return pl;
}

// columns per workgroup of tnet_patch_gemm_kernel: as wide as possible while the grid still covers the chip
inline int patch_nt(int tiles, int cols) {
    int nt = cols <= 32 ? 2 : 4;
    while (nt > 2 && (int64_t)tiles * ((cols + 16 * nt - 1) / (16 * nt)) < 256) nt >>= 1;
    return nt;
}
inline size_t patch_lds(int NT) { return 2 * (S * TP * LDK + S * 16 * NT * LDK) * 2; }

template <bool DX>
int launch_gemm(const PDesc& d, const float* src, const float* w, float* dst, hipStream_t s) {
    const int tiles = (d.P + TP - 1) / TP, cols = DX ? d.K : d.C_out;
    const int NT = patch_nt(tiles, cols);
    const dim3 grid(tiles, (cols + 16 * NT - 1) / (16 * NT));
    const size_t lds = patch_lds(NT);
    if (NT == 2) {
        hipLaunchKernelGGL((tnet_patch_gemm_kernel<2, DX>), grid, dim3(256), lds, s, src, w, dst, d);
    } else {
        const int rc = tnet_raise_lds(tnet_patch_gemm_kernel<4, DX>, lds);
        if (rc != GHN3_OK) return rc;
        hipLaunchKernelGGL((tnet_patch_gemm_kernel<4, DX>), grid, dim3(256), lds, s, src, w, dst, d);
    }
    TNET_LAUNCH_CHECK("tnet patch gemm");
    return GHN3_OK;
}

}  // namespace

extern "C" int64_t ghn3_patch_scratch_floats(const ghn3_patch_desc* g, int backward) {
    PDesc d;
    const int rc = check_pdesc(g, d);
    if (rc != GHN3_OK) return rc;
    if (!backward) return 0;
    const PPlan pl = make_pplan(d);
    return pl.chunks > 1 ? al((int64_t)pl.chunks * d.C_out * d.K) : 0;
}

extern "C" int ghn3_patch_fwd(const ghn3_patch_desc* g, const float* x, const float* w, float* z, float* scratch, void* stream_) {
    PDesc d;
    const int rc = check_pdesc(g, d);
    if (rc != GHN3_OK) return rc;
    (void)scratch;
    if (!x || !w || !z) { ghn3_set_error("patch fwd: null operand"); return GHN3_E_ARG; }
    return launch_gemm<false>(d, x, w, z, (hipStream_t)stream_);
}

extern "C" int ghn3_patch_bwd(const ghn3_patch_desc* g, const float* dz, const float* x, const float* w, float* dx, float* dw,
                              float* scratch, void* stream_) {
    PDesc d;
    int rc = check_pdesc(g, d);
    if (rc != GHN3_OK) return rc;
    hipStream_t s = (hipStream_t)stream_;
    const PPlan pl = make_pplan(d);
    if (!dz || (dw && !x) || (dx && !w) || (dw && pl.chunks > 1 && !scratch)) {
        ghn3_set_error("patch bwd: null operand");
        return GHN3_E_ARG;
    }
    if (dx) {
        if ((rc = launch_gemm<true>(d, dz, w, dx, s)) != GHN3_OK) return rc;
        const bool gaps = d.sh != d.kh || d.sw != d.kw || (d.Ho - 1) * d.sh + d.kh != d.H || (d.Wo - 1) * d.sw + d.kw != d.W;
        if (gaps) {
            const int64_t total = (int64_t)d.N * d.C_in * d.H * d.W;
            const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
            hipLaunchKernelGGL(tnet_patch_gaps_kernel, dim3(blocks), dim3(256), 0, s, dx, d, total);
            TNET_LAUNCH_CHECK("tnet patch gaps");
        }
    }
    if (dw) {
        float* out = pl.chunks > 1 ? scratch : dw;
        hipLaunchKernelGGL(tnet_patch_wgrad_kernel, dim3(pl.tiles * pl.chunks), dim3(256), 0, s, dz, x, out, d, pl.chunks, pl.chunk_px,
                           pl.tiles_n);
        TNET_LAUNCH_CHECK("tnet patch wgrad");
        if (pl.chunks > 1) {
            const TnetRedProb red{scratch, dw, nullptr, pl.chunks, d.C_out * d.K, d.K, d.K, 0};
            if ((rc = tnet_reduce_launch(&red, 1, s)) != GHN3_OK) return rc;
        }
    }
    return GHN3_OK;
}
