// The glue of a target-network cell on the op family's storage (include/ghn3_hip.h, "target-network joins"): the sum of two
// branch outputs, the concatenation of a cell's states and the positional encoding of the ViT-style networks, forward and
// backward.  Plain fp32 and bandwidth-bound: one lane moves four channels (16 bytes), and the lanes of a wave run along the axis
// that is contiguous in the tensor being WRITTEN (channels for NHWC, pixels for NCHW), so every store is coalesced and so is
// every load from a tensor of the same layout.  A load from a tensor of the other layout is one 16-byte piece per lane (NHWC
// source) or four 4-byte pieces (NCHW source) and leans on the L2; the training loop's light networks never take that path
// (all of their activations are NHWC), so it has no LDS transpose of its own.  No atomics, no scratch memory: every output
// element has exactly one writer, and each is one fp32 add or a copy, so the results are exact.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "tnet_common.h"

namespace {

constexpr int JOIN_THREADS = 256;
constexpr int JOIN_MAX_BLOCKS = 8192;
constexpr int64_t JOIN_MAX_ELEMS = (int64_t)1 << 31;

// four consecutive channels c .. c + 3 of pixel (n, h, w) of a dense (N, C, H, W) tensor in either layout
__device__ inline f32x4 load4(const float* p, int layout, int C, int H, int W, int n, int c, int h, int w) {
    if (layout) return *(const f32x4*)(p + (((int64_t)n * H + h) * W + w) * C + c);
    const int64_t plane = (int64_t)H * W;
    const float* q = p + ((int64_t)n * C + c) * plane + (int64_t)h * W + w;
    return f32x4{q[0], q[plane], q[2 * plane], q[3 * plane]};
}

__device__ inline void store4(float* p, int layout, int C, int H, int W, int n, int c, int h, int w, f32x4 v) {
    if (layout) {
        *(f32x4*)(p + (((int64_t)n * H + h) * W + w) * C + c) = v;
        return;
    }
    const int64_t plane = (int64_t)H * W;
    float* q = p + ((int64_t)n * C + c) * plane + (int64_t)h * W + w;
    q[0] = v.x; q[plane] = v.y; q[2 * plane] = v.z; q[3 * plane] = v.w;
}

// work item l of a dense (N, C, H, W) tensor of Q = C / 4 channel quads -> (n, quad, h, w), the quads running fastest for NHWC
// and the pixels for NCHW
__device__ inline void item_of(uint32_t l, int layout, int Q, int H, int W, int& n, int& q, int& h, int& w) {
    const uint32_t HW = (uint32_t)H * W;
    uint32_t pix;
    if (layout) {
        q = (int)(l % Q);
        pix = l / Q;
        n = (int)(pix / HW);
        pix %= HW;
    } else {
        pix = l % HW;
        const uint32_t r = l / HW;
        q = (int)(r % Q);
        n = (int)(r / Q);
    }
    h = (int)(pix / W);
    w = (int)(pix % W);
}

__device__ inline f32x4 load_src(const ghn3_join_src& s, int C, int n, int c, int h, int w) {
    return load4(s.p, s.layout, C, s.H, s.W, s.broadcast_n ? 0 : n, c, h * s.step, w * s.step);
}

__global__ __launch_bounds__(JOIN_THREADS) void tnet_join_fwd_kernel(ghn3_join_desc d, float* __restrict__ out, uint32_t total) {
    const int Q = d.C / 4;
    for (uint32_t t = blockIdx.x * JOIN_THREADS + threadIdx.x; t < total; t += gridDim.x * JOIN_THREADS) {
        int n, q, h, w;
        item_of(t, d.layout, Q, d.H, d.W, n, q, h, w);
        const int c = 4 * q;
        int j = 0;
        while (j + 1 < d.n_slices && c >= d.s[j + 1].c0) ++j;
        const ghn3_join_slice& sl = d.s[j];
        f32x4 v = load_src(sl.a, sl.C, n, c - sl.c0, h, w);
        if (sl.b.p) v += load_src(sl.b, sl.C, n, c - sl.c0, h, w);
        store4(out, d.layout, d.C, d.H, d.W, n, c, h, w, v);
    }
}

// one gradient tensor of the backward: a dense (N, C, H, W) tensor in `layout`, fed by channels [c0, c0 + C) of dout at its
// pixels (h step, w step); work items [start, start of the next entry)
struct GradEnt {
    float* g;
    int64_t start;
    int32_t H, W, C, c0, step, layout;
};
struct GradTable {
    GradEnt e[2 * GHN3_JOIN_MAX_SLICES];
    int32_t n_ent, N, H, W, C, layout;      // (N, C, H, W), layout: dout's
};

__global__ __launch_bounds__(JOIN_THREADS) void tnet_join_bwd_kernel(GradTable tb, const float* __restrict__ dout, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * JOIN_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * JOIN_THREADS) {
        int j = 0;
        while (j + 1 < tb.n_ent && t >= tb.e[j + 1].start) ++j;
        const GradEnt& e = tb.e[j];
        int n, q, h, w;
        item_of((uint32_t)(t - e.start), e.layout, e.C / 4, e.H, e.W, n, q, h, w);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e.step == 1 || !((h | w) & 1))             // (a pixel the strided read skipped keeps the zero)
            v = load4(dout, tb.layout, tb.C, tb.H, tb.W, n, e.c0 + 4 * q, h / e.step, w / e.step);
        store4(e.g, e.layout, e.C, e.H, e.W, n, 4 * q, h, w, v);
    }
}

// dw [C][H][W] = sum over n of dy (N, C, H, W) in `layout`, n = 0, 1, ... in that order; one lane per (h, w, four channels)
__global__ __launch_bounds__(JOIN_THREADS) void tnet_posenc_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dw, int N,
                                                                       int C, int H, int W, int layout, uint32_t total) {
    for (uint32_t t = blockIdx.x * JOIN_THREADS + threadIdx.x; t < total; t += gridDim.x * JOIN_THREADS) {
        int n0, q, h, w;
        item_of(t, layout, C / 4, H, W, n0, q, h, w);   // (total covers one image: n0 == 0)
        f32x4 acc = load4(dy, layout, C, H, W, 0, 4 * q, h, w);
        for (int n = 1; n < N; ++n) acc += load4(dy, layout, C, H, W, n, 4 * q, h, w);
        store4(dw, 0, C, H, W, 0, 4 * q, h, w, acc);
    }
}

int grid_for(int64_t total) { return (int)std::min<int64_t>((total + JOIN_THREADS - 1) / JOIN_THREADS, JOIN_MAX_BLOCKS); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// one source of slice j (C channels) against the output map of d; `ptr` = the pointer this direction reads or writes
int check_src(const ghn3_join_desc& d, int j, const char* which, const ghn3_join_src& s, int C, const void* ptr) {
    if (s.step != 1 && s.step != 2) { ghn3_set_error("join: slice %d source %s: step %d is neither 1 nor 2", j, which, s.step); return GHN3_E_ARG; }
    if (s.layout != 0 && s.layout != 1) { ghn3_set_error("join: slice %d source %s: layout %d is neither 0 (NCHW) nor 1 (NHWC)", j, which, s.layout); return GHN3_E_ARG; }
    if (s.H <= 0 || s.W <= 0 || (s.H + s.step - 1) / s.step != d.H || (s.W + s.step - 1) / s.step != d.W) {
        ghn3_set_error("join: slice %d source %s: map %d x %d at step %d is not the output's %d x %d", j, which, s.H, s.W, s.step, d.H, d.W);
        return GHN3_E_ARG;
    }
    if ((int64_t)(s.broadcast_n ? 1 : d.N) * C * s.H * s.W >= JOIN_MAX_ELEMS) {
        ghn3_set_error("join: slice %d source %s: tensors of 2^31 elements or more are not supported", j, which);
        return GHN3_E_LIMIT;
    }
    if (s.layout && !aligned16(ptr)) { ghn3_set_error("join: slice %d source %s: an NHWC tensor must start on 16 bytes", j, which); return GHN3_E_ARG; }
    return GHN3_OK;
}

int check_desc(const ghn3_join_desc* g, const void* out) {
    if (!g) { ghn3_set_error("join: null descriptor"); return GHN3_E_ARG; }
    const ghn3_join_desc& d = *g;
    if (d.N <= 0 || d.H <= 0 || d.W <= 0 || d.C <= 0) { ghn3_set_error("join: non-positive size in the descriptor"); return GHN3_E_ARG; }
    if (d.layout != 0 && d.layout != 1) { ghn3_set_error("join: layout %d is neither 0 (NCHW) nor 1 (NHWC)", d.layout); return GHN3_E_ARG; }
    if (d.n_slices < 1 || d.n_slices > GHN3_JOIN_MAX_SLICES) {
        ghn3_set_error("join: %d slices (1 .. %d are supported)", d.n_slices, GHN3_JOIN_MAX_SLICES);
        return GHN3_E_LIMIT;
    }
    if (!out) { ghn3_set_error("join: null pointer"); return GHN3_E_ARG; }
    if (d.layout && !aligned16(out)) { ghn3_set_error("join: an NHWC tensor must start on 16 bytes"); return GHN3_E_ARG; }
    int64_t c0 = 0;
    for (int j = 0; j < d.n_slices; ++j) {
        const ghn3_join_slice& s = d.s[j];
        if (s.C <= 0 || s.c0 != c0) { ghn3_set_error("join: slice %d (c0 %d, C %d) does not continue the slices before it", j, s.c0, s.C); return GHN3_E_ARG; }
        if (s.C % 4 || s.c0 % 4) { ghn3_set_error("join: slice %d: C %d and c0 %d must be multiples of 4", j, s.C, s.c0); return GHN3_E_LIMIT; }
        c0 += s.C;
    }
    if (c0 != d.C) { ghn3_set_error("join: the slices cover %lld channels of %d", (long long)c0, d.C); return GHN3_E_ARG; }
    if ((int64_t)d.N * d.C * d.H * d.W >= JOIN_MAX_ELEMS) { ghn3_set_error("join: tensors of 2^31 elements or more are not supported"); return GHN3_E_LIMIT; }
    return GHN3_OK;
}

}  // namespace

extern "C" int ghn3_join_fwd(const ghn3_join_desc* desc, float* out, void* stream) {
    int rc = check_desc(desc, out);
    if (rc) return rc;
    const ghn3_join_desc& d = *desc;
    for (int j = 0; j < d.n_slices; ++j) {
        const ghn3_join_slice& s = d.s[j];
        if (!s.a.p) { ghn3_set_error("join fwd: slice %d has no source", j); return GHN3_E_ARG; }
        if ((rc = check_src(d, j, "a", s.a, s.C, s.a.p))) return rc;
        if (s.b.p && (rc = check_src(d, j, "b", s.b, s.C, s.b.p))) return rc;
    }
    const int64_t total = (int64_t)d.N * d.H * d.W * (d.C / 4);
    hipLaunchKernelGGL(tnet_join_fwd_kernel, dim3(grid_for(total)), dim3(JOIN_THREADS), 0, (hipStream_t)stream, d, out, (uint32_t)total);
    TNET_LAUNCH_CHECK("join fwd")
    return GHN3_OK;
}

extern "C" int ghn3_join_bwd(const ghn3_join_desc* desc, const float* dout, void* stream) {
    int rc = check_desc(desc, dout);
    if (rc) return rc;
    const ghn3_join_desc& d = *desc;
    GradTable tb{};
    tb.N = d.N; tb.H = d.H; tb.W = d.W; tb.C = d.C; tb.layout = d.layout;
    int64_t total = 0;
    for (int j = 0; j < d.n_slices; ++j) {
        const ghn3_join_slice& s = d.s[j];
        const ghn3_join_src* both[2] = {&s.a, &s.b};
        for (int k = 0; k < 2; ++k) {
            const ghn3_join_src& src = *both[k];
            if (!src.grad) continue;
            if (src.broadcast_n) { ghn3_set_error("join bwd: slice %d: the gradient of a batch-broadcast source is ghn3_posenc_bwd's", j); return GHN3_E_ARG; }
            if ((rc = check_src(d, j, k ? "b" : "a", src, s.C, src.grad))) return rc;
            tb.e[tb.n_ent++] = GradEnt{src.grad, total, src.H, src.W, s.C, s.c0, src.step, src.layout};
            total += (int64_t)d.N * src.H * src.W * (s.C / 4);
        }
    }
    if (!tb.n_ent) return GHN3_OK;
    hipLaunchKernelGGL(tnet_join_bwd_kernel, dim3(grid_for(total)), dim3(JOIN_THREADS), 0, (hipStream_t)stream, tb, dout, total);
    TNET_LAUNCH_CHECK("join bwd")
    return GHN3_OK;
}

extern "C" int ghn3_posenc_bwd(int N, int C, int H, int W, int layout, const float* dy, float* dw, void* stream) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) { ghn3_set_error("posenc bwd: non-positive size"); return GHN3_E_ARG; }
    if (layout != 0 && layout != 1) { ghn3_set_error("posenc bwd: layout %d is neither 0 (NCHW) nor 1 (NHWC)", layout); return GHN3_E_ARG; }
    if (!dy || !dw) { ghn3_set_error("posenc bwd: null pointer"); return GHN3_E_ARG; }
    if (C % 4) { ghn3_set_error("posenc bwd: C %d must be a multiple of 4", C); return GHN3_E_LIMIT; }
    if ((int64_t)N * C * H * W >= JOIN_MAX_ELEMS) { ghn3_set_error("posenc bwd: tensors of 2^31 elements or more are not supported"); return GHN3_E_LIMIT; }
    if (layout && !aligned16(dy)) { ghn3_set_error("posenc bwd: an NHWC tensor must start on 16 bytes"); return GHN3_E_ARG; }
    const int64_t total = (int64_t)H * W * (C / 4);
    hipLaunchKernelGGL(tnet_posenc_bwd_kernel, dim3(grid_for(total)), dim3(JOIN_THREADS), 0, (hipStream_t)stream, dy, dw, N, C, H, W, layout,
                       (uint32_t)total);
    TNET_LAUNCH_CHECK("posenc bwd")
    return GHN3_OK;
}
