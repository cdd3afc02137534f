// Target-network layers: the weight (+ bias) gradients of every linear layer of the msa op (tnet_msa.hip) and of the classifier
// head (tnet_head.hip), and the fixed-order sums that finish them.
//
//   tnet_wgrad    dW [Nout][K] = G^T X (db [Nout] = column sums of G, as column K of an X padded with ones) for up to four
//                 linears in one launch: a workgroup per WG_ROWS-row chunk and 32 x 32 output block, a wave per 16 x 16
//                 quarter; the chunk's product goes to its slot of the partials, or straight to w / b when the caller has one
//                 chunk and passes no partials;
//   tnet_reduce   one thread per element: sums the partials (and the LayerNorm-parameter partials of the msa kernels) in part
//                 order -> dense gradients.
//
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate): the four instructions of a 16-row step take rows
// r0 + 4 (lane >> 4) + j.  No float atomics: reruns are bit-identical.

#include "tnet_common.h"

namespace {

constexpr int NT = 256;                     // threads per workgroup (4 waves)
constexpr int WG_ROWS = 256;                // rows per partial product

struct WgSet {
    TnetWgProb p[TNET_WG_MAX];
    int tiles_n[TNET_WG_MAX], tiles_k[TNET_WG_MAX], chunks[TNET_WG_MAX], block_start[TNET_WG_MAX];
    int n;
};

__global__ __launch_bounds__(NT) void tnet_wgrad_kernel(WgSet set) {
    int pi = 0;
    for (int j = 1; j < set.n; ++j) pi = (int)blockIdx.x >= set.block_start[j] ? j : pi;
    const TnetWgProb& P = set.p[pi];
    const int chunks = set.chunks[pi], tiles_n = set.tiles_n[pi];
    const int local = blockIdx.x - set.block_start[pi];
    const int chunk = local % chunks, tile = local / chunks;
    const int tn = tile % tiles_n, tk = tile / tiles_n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int n0 = tn * 32 + (wave & 1) * 16, k0 = tk * 32 + (wave >> 1) * 16;
    const int K1 = P.K + P.bias;
    const int n = n0 + i, k = k0 + i;
    const bool nok = n < P.Nout, kok = k < K1;
    const int nc = nok ? n : 0, kc = k < P.K ? k : 0;
    const int rb = chunk * WG_ROWS, re = min(rb + WG_ROWS, P.rows);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r0 = rb; r0 < re; r0 += 16) {
        float a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = r0 + 4 * q + j;
            const bool rok = r < re;
            const int rc = rok ? r : rb;
            const float gv = P.G[(size_t)rc * P.Nout + nc];
            const float xv = k < P.K ? P.X[(size_t)rc * P.K + kc] : 1.f;
            a[j] = (rok && nok) ? gv : 0.f;
            b[j] = (rok && kok) ? xv : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
    }
    // C/D: row (n) 4 q + g, col (k) i
    if (kok) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int nn = n0 + 4 * q + g;
            if (nn >= P.Nout) continue;
            if (P.part) P.part[((size_t)chunk * P.Nout + nn) * K1 + k] = acc[g];
            else if (k < P.K) P.w[(size_t)nn * P.K + k] = acc[g];
            else P.b[nn] = acc[g];
        }
    }
}

struct RedSet { TnetRedProb p[TNET_RED_MAX]; int block_start[TNET_RED_MAX]; int n; };

__global__ __launch_bounds__(NT) void tnet_reduce_kernel(RedSet set) {
    int pi = 0;
    for (int j = 1; j < set.n; ++j) pi = (int)blockIdx.x >= set.block_start[j] ? j : pi;
    const TnetRedProb& P = set.p[pi];
    const int e = (blockIdx.x - set.block_start[pi]) * NT + threadIdx.x;
    if (e >= P.M) return;
    float s = 0.f;
    for (int c = 0; c < P.parts; ++c) s += P.part[(size_t)c * P.M + e];
    if (P.ln) {
        if (e < P.K) P.w[e] = s; else P.b[e - P.K] = s;
    } else {
        const int n = e / P.ld, k = e - n * P.ld;
        if (k < P.K) P.w[(size_t)n * P.K + k] = s;
        else if (P.b) P.b[n] = s;
    }
}

}  // namespace

int tnet_wg_chunks(int rows) { return (rows + WG_ROWS - 1) / WG_ROWS; }
int64_t tnet_wg_part_floats(int rows, int Nout, int K) { return al((int64_t)tnet_wg_chunks(rows) * Nout * (K + 1)); }

int tnet_wgrad_launch(const TnetWgProb* probs, int n, hipStream_t s) {
    if (n < 1 || n > TNET_WG_MAX) { ghn3_set_error("tnet wgrad: %d problems (1 .. %d)", n, TNET_WG_MAX); return GHN3_E_ARG; }
    WgSet ws;
    ws.n = n;
    int blocks = 0;
    for (int j = 0; j < n; ++j) {
        const TnetWgProb& q = probs[j];
        ws.p[j] = q;
        ws.tiles_n[j] = (q.Nout + 31) / 32;
        ws.tiles_k[j] = (q.K + q.bias + 31) / 32;
        ws.chunks[j] = tnet_wg_chunks(q.rows);
        ws.block_start[j] = blocks;
        blocks += ws.tiles_n[j] * ws.tiles_k[j] * ws.chunks[j];
        const bool in_place = ws.chunks[j] == 1 && q.w && (q.b || !q.bias);
        if (!q.G || !q.X || (!q.part && !in_place)) {
            ghn3_set_error("tnet wgrad: problem %d has a null operand, or neither partials nor a single chunk with w / b", j);
            return GHN3_E_ARG;
        }
    }
    hipLaunchKernelGGL(tnet_wgrad_kernel, dim3(blocks), dim3(NT), 0, s, ws);
    TNET_LAUNCH_CHECK("tnet wgrad");
    return GHN3_OK;
}

int tnet_reduce_launch(const TnetRedProb* probs, int n, hipStream_t s) {
    if (n < 1 || n > TNET_RED_MAX) { ghn3_set_error("tnet reduce: %d problems (1 .. %d)", n, TNET_RED_MAX); return GHN3_E_ARG; }
    RedSet rs;
    rs.n = n;
    int blocks = 0;
    for (int j = 0; j < n; ++j) {
        rs.p[j] = probs[j];
        rs.block_start[j] = blocks;
        blocks += (probs[j].M + NT - 1) / NT;
    }
    hipLaunchKernelGGL(tnet_reduce_kernel, dim3(blocks), dim3(NT), 0, s, rs);
    TNET_LAUNCH_CHECK("tnet reduce");
    return GHN3_OK;
}
