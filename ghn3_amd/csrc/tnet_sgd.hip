// The optimizer step of a plain network (include/ghn3_hip.h, "multi-tensor SGD step"): clip_grad_norm_ + torch.optim.SGD over a
// table of separate parameter / gradient / momentum tensors in two launches.  Streaming and HBM-bound: the norm pass reads 4
// bytes per parameter, the update reads 12 and writes 8.  A ResNet-50 has 161 tensors, half of them BatchNorm vectors of 64 to
// 2048 floats, so the work list is cut into chunks of GHN3_MT_CHUNK elements of ONE tensor each and a workgroup strides over the
// chunks: large tensors spread over the whole chip, small ones cost one workgroup visit each.
//
// One code path for the arithmetic: a lane always works on a quad (four consecutive elements, 4 q .. 4 q + 3 counted from the
// tensor's start).  Only the loads and stores differ -- one 16-byte access when the tensor is aligned and the quad is whole, else
// up to four 4-byte ones with the missing elements read as zero and not stored -- so an aligned tensor and a view 4 bytes into a
// buffer give the same bits, and so does the norm.  Every product that feeds a sum is an explicit fused multiply-add: nothing is
// left for the compiler to contract one way here and another way there.  No atomics.

#include <hip/hip_runtime.h>

#include "tnet_common.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_MAX_BLOCKS = 2048;
constexpr int MT_QUADS = GHN3_MT_CHUNK / 4;           // quads of a full chunk
static_assert(GHN3_MT_CHUNK % (4 * MT_THREADS) == 0, "a full chunk is a whole number of workgroup passes");

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// elements [0, cnt) of the quad at q (cnt = 4: the whole quad); missing elements read as zero
__device__ __forceinline__ f32x4 load_quad(const float* q, bool vec, int cnt) {
    if (vec && cnt == 4) return *reinterpret_cast<const f32x4*>(q);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (cnt > 0) v.x = q[0];
    if (cnt > 1) v.y = q[1];
    if (cnt > 2) v.z = q[2];
    if (cnt > 3) v.w = q[3];
    return v;
}
__device__ __forceinline__ void store_quad(float* q, bool vec, int cnt, f32x4 v) {
    if (vec && cnt == 4) { *reinterpret_cast<f32x4*>(q) = v; return; }
    if (cnt > 0) q[0] = v.x;
    if (cnt > 1) q[1] = v.y;
    if (cnt > 2) q[2] = v.z;
    if (cnt > 3) q[3] = v.w;
}

// parts[c] = sum of squares of chunk c's gradient.  A lane's quads, the wave butterfly and the sum of the four waves are fixed by
// the chunk alone, not by the grid.
__global__ __launch_bounds__(MT_THREADS) void mt_sumsq_kernel(const ghn3_mt_tensor* __restrict__ tensors,
                                                              const float* const* __restrict__ grads,
                                                              const ghn3_mt_chunk* __restrict__ chunks, int n_chunks,
                                                              float* __restrict__ parts) {
    __shared__ float part[MT_THREADS / 64];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ghn3_mt_chunk ch = chunks[c];
        const int64_t left = tensors[ch.tensor].n - ch.first;
        const int len = left < GHN3_MT_CHUNK ? (int)left : GHN3_MT_CHUNK;
        const float* g = grads[ch.tensor] + ch.first;
        const bool vec = aligned16(g);
        float acc = 0.f;
        for (int q = threadIdx.x; 4 * q < len; q += MT_THREADS) {
            const f32x4 v = load_quad(g + 4 * q, vec, len - 4 * q < 4 ? len - 4 * q : 4);
            acc = __builtin_fmaf(v.x, v.x, acc);
            acc = __builtin_fmaf(v.y, v.y, acc);
            acc = __builtin_fmaf(v.z, v.z, acc);
            acc = __builtin_fmaf(v.w, v.w, acc);
        }
        acc = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) parts[c] = (part[0] + part[1]) + (part[2] + part[3]);
        __syncthreads();                                // (part[] is written again for the workgroup's next chunk)
    }
}

// out[0] = the partials added in a fixed order: lane t takes parts[t], parts[t + 256], ...; lane 0 adds the 256 sums in order
__global__ __launch_bounds__(MT_THREADS) void mt_sumsq_finish_kernel(float* __restrict__ out, const float* __restrict__ parts,
                                                                     int n) {
    __shared__ float tot[MT_THREADS];
    float acc = 0.f;
    for (int k = threadIdx.x; k < n; k += MT_THREADS) acc += parts[k];
    tot[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < MT_THREADS; ++k) t += tot[k];
        out[0] = t;
    }
}

// one element of torch.optim.SGD on the clipped, unscaled gradient; m is not touched when momentum == 0
__device__ __forceinline__ void sgd_element(float& p, float g, float& m, const ghn3_mt_sgd_args& a, float coef) {
    const float d = __builtin_fmaf(g, coef, a.weight_decay * p);
    float u = d;
    if (a.momentum != 0.f) {
        m = __builtin_fmaf(a.momentum, m, d);
        u = a.nesterov ? __builtin_fmaf(a.momentum, m, d) : m;
    }
    p = __builtin_fmaf(-a.lr, u, p);
}

__global__ __launch_bounds__(MT_THREADS) void mt_sgd_kernel(const ghn3_mt_tensor* __restrict__ tensors,
                                                            const float* const* __restrict__ grads,
                                                            const ghn3_mt_chunk* __restrict__ chunks, int n_chunks,
                                                            const float* __restrict__ sumsq, ghn3_mt_sgd_args a) {
    // Non-finite gradient norm (an inf / NaN in any gradient, e.g. an fp16 overflow under AMP): no parameter and no momentum
    // buffer changes, like GradScaler's found_inf, without a host round trip -- the guard of adamw_body.
    if (sumsq && !isfinite(*sumsq)) return;
    float coef = a.inv_scale;
    if (sumsq && a.max_norm > 0.f)
        coef = a.inv_scale * fminf(1.f, a.max_norm / __builtin_fmaf(sqrtf(*sumsq), a.inv_scale, 1e-6f));
    const bool has_m = a.momentum != 0.f;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ghn3_mt_chunk ch = chunks[c];
        const ghn3_mt_tensor t = tensors[ch.tensor];
        const int64_t left = t.n - ch.first;
        const int len = left < GHN3_MT_CHUNK ? (int)left : GHN3_MT_CHUNK;
        float* p = t.p + ch.first;
        float* m = has_m ? t.m + ch.first : nullptr;
        const float* g = grads[ch.tensor] + ch.first;
        const bool vec = aligned16(p) && aligned16(g) && aligned16(m);
        for (int q = threadIdx.x; 4 * q < len; q += MT_THREADS) {
            const int cnt = len - 4 * q < 4 ? len - 4 * q : 4;
            f32x4 pv = load_quad(p + 4 * q, vec, cnt);
            const f32x4 gv = load_quad(g + 4 * q, vec, cnt);
            f32x4 mv = {0.f, 0.f, 0.f, 0.f};
            if (has_m) mv = load_quad(m + 4 * q, vec, cnt);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pv[e], me = mv[e];
                sgd_element(pe, gv[e], me, a, coef);
                pv[e] = pe; mv[e] = me;
            }
            if (has_m) store_quad(m + 4 * q, vec, cnt, mv);
            store_quad(p + 4 * q, vec, cnt, pv);
        }
    }
}

// Gather / scatter between the table's separate tensors and their segments of ONE flat buffer (ghn3_mt_pack / ghn3_mt_unpack):
// bit copies over the same chunk list and with the same quad accesses as the step above.  PACK: other[k] -> segs[k].p, else
// segs[k].p -> other[k]; elements [0, n) only, so a segment's pad floats and everything around a tensor stay as they are.
template <bool PACK>
__global__ __launch_bounds__(MT_THREADS) void mt_wire_kernel(const ghn3_mt_tensor* __restrict__ segs,
                                                             float* const* __restrict__ other,
                                                             const ghn3_mt_chunk* __restrict__ chunks, int n_chunks) {
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ghn3_mt_chunk ch = chunks[c];
        const ghn3_mt_tensor t = segs[ch.tensor];
        const int64_t left = t.n - ch.first;
        const int len = left < GHN3_MT_CHUNK ? (int)left : GHN3_MT_CHUNK;
        float* flat = t.p + ch.first;
        float* sep = other[ch.tensor] + ch.first;
        const float* src = PACK ? sep : flat;
        float* dst = PACK ? flat : sep;
        const bool vec = aligned16(src) && aligned16(dst);
        for (int q = threadIdx.x; 4 * q < len; q += MT_THREADS) {
            const int cnt = len - 4 * q < 4 ? len - 4 * q : 4;
            store_quad(dst + 4 * q, vec, cnt, load_quad(src + 4 * q, vec, cnt));
        }
    }
}

int check_tables(const char* what, const void* tensors, const void* grads, const void* chunks, int n_chunks) {
    if (n_chunks < 0) { ghn3_set_error("%s: %d chunks", what, n_chunks); return GHN3_E_ARG; }
    if (n_chunks == 0) return GHN3_OK;
    if (!tensors || !grads || !chunks) { ghn3_set_error("%s: null table", what); return GHN3_E_ARG; }
    if ((reinterpret_cast<uintptr_t>(tensors) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(chunks)) & 7) {
        ghn3_set_error("%s: the tables must start on 8 bytes", what);
        return GHN3_E_ARG;
    }
    return GHN3_OK;
}

}  // namespace

extern "C" int ghn3_mt_sumsq(const ghn3_mt_tensor* tensors, const float* const* grads, const ghn3_mt_chunk* chunks, int n_chunks,
                             float* parts, float* out, void* stream) {
    const int rc = check_tables("mt_sumsq", tensors, grads, chunks, n_chunks);
    if (rc) return rc;
    if (!out || (n_chunks > 0 && !parts)) { ghn3_set_error("mt_sumsq: null pointer"); return GHN3_E_ARG; }
    if (n_chunks > 0) {
        const int grid = n_chunks < MT_MAX_BLOCKS ? n_chunks : MT_MAX_BLOCKS;
        hipLaunchKernelGGL(mt_sumsq_kernel, dim3(grid), dim3(MT_THREADS), 0, (hipStream_t)stream, tensors, grads, chunks, n_chunks, parts);
        TNET_LAUNCH_CHECK("mt_sumsq")
    }
    hipLaunchKernelGGL(mt_sumsq_finish_kernel, dim3(1), dim3(MT_THREADS), 0, (hipStream_t)stream, out, parts, n_chunks);
    TNET_LAUNCH_CHECK("mt_sumsq finish")
    return GHN3_OK;
}

extern "C" int ghn3_mt_sgd(const ghn3_mt_tensor* tensors, const float* const* grads, const ghn3_mt_chunk* chunks, int n_chunks,
                           const float* sumsq, const ghn3_mt_sgd_args* args, void* stream) {
    const int rc = check_tables("mt_sgd", tensors, grads, chunks, n_chunks);
    if (rc) return rc;
    if (!args) { ghn3_set_error("mt_sgd: null arguments"); return GHN3_E_ARG; }
    ghn3_mt_sgd_args a = *args;
    if (a.nesterov && a.momentum == 0.f) { ghn3_set_error("mt_sgd: nesterov needs a momentum"); return GHN3_E_ARG; }
    if (!(a.inv_scale > 0.f)) a.inv_scale = 1.f;
    if (n_chunks == 0) return GHN3_OK;
    const int grid = n_chunks < MT_MAX_BLOCKS ? n_chunks : MT_MAX_BLOCKS;
    hipLaunchKernelGGL(mt_sgd_kernel, dim3(grid), dim3(MT_THREADS), 0, (hipStream_t)stream, tensors, grads, chunks, n_chunks, sumsq, a);
    TNET_LAUNCH_CHECK("mt_sgd")
    return GHN3_OK;
}

extern "C" int ghn3_mt_pack(const ghn3_mt_tensor* segs, const float* const* src, const ghn3_mt_chunk* chunks, int n_chunks,
                            void* stream) {
    const int rc = check_tables("mt_pack", segs, src, chunks, n_chunks);
    if (rc || n_chunks == 0) return rc;
    const int grid = n_chunks < MT_MAX_BLOCKS ? n_chunks : MT_MAX_BLOCKS;
    hipLaunchKernelGGL(mt_wire_kernel<true>, dim3(grid), dim3(MT_THREADS), 0, (hipStream_t)stream, segs,
                       const_cast<float* const*>(src), chunks, n_chunks);
    TNET_LAUNCH_CHECK("mt_pack")
    return GHN3_OK;
}

extern "C" int ghn3_mt_unpack(const ghn3_mt_tensor* segs, float* const* dst, const ghn3_mt_chunk* chunks, int n_chunks,
                              void* stream) {
    const int rc = check_tables("mt_unpack", segs, dst, chunks, n_chunks);
    if (rc || n_chunks == 0) return rc;
    const int grid = n_chunks < MT_MAX_BLOCKS ? n_chunks : MT_MAX_BLOCKS;
    hipLaunchKernelGGL(mt_wire_kernel<false>, dim3(grid), dim3(MT_THREADS), 0, (hipStream_t)stream, segs, dst, chunks, n_chunks);
    TNET_LAUNCH_CHECK("mt_unpack")
    return GHN3_OK;
}
