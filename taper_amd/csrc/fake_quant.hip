// fake_quant.hip -- quantization-aware training's fake quantization (src/quantization/fake_quantize.rs, done as the reference means it):
// a tensor goes through a quantization codec and straight back to f32, so that training sees the rounding a later quantize() adds.
//
//   th_fake_quant_multi  weights: the storage codecs of quant.hip as a round trip (int8: finite min / max -> {min_val, scale} -> codes ->
//                        dequant_int8; f16: the reference's half codec both ways), every tensor of a list in TWO launches -- a min / max
//                        pass over the int8 tensors, then one pass that folds each tensor's partials and writes its round trip
//   th_fake_quant_act    one activation tensor: int8 symmetric per tensor with the scale of this batch (fake_quantize.rs:71-118,
//                        155-162), f16 the half round trip; two launches (int8) or one (f16)
//
// Both are HBM streams: 16-byte loads and stores per lane, grids sized to the CUs (not to n) with grid-stride loops, and the per-workgroup
// min / max partials folded by every applying workgroup in the same order.  Min / max are exact, so the fold gives the same bits in any
// order; the codecs themselves are quant_dev.h's, so the results are bit-identical to th_quantize_int8 + th_dequantize_int8 / the f16
// pair.  No host synchronisation, no host-side reads of the descriptors: both calls can be captured into a graph.
#include "common.h"
#include "quant_dev.h"

namespace th {

constexpr int kFqThreads = 256;
constexpr int kFqParts = 512;                   // workgroups of the min / max pass (2 per CU): the most partials a tensor leaves
constexpr int kFqApply = 1024;                  // workgroups of the applying pass (4 per CU)
constexpr int64_t kFqPartMin = 4 * 256 * 8;     // elements per min / max workgroup at least (8 float4 loads per lane)
constexpr int64_t kFqApplyMin = 4 * 256;        // ... per applying workgroup (one float4 per lane)

__host__ __device__ __forceinline__ int fq_spread(int64_t n, int64_t per, int most) {   // workgroups for n elements, >= per each, <= most
    const int64_t k = (n + per - 1) / per;
    return (int)(k < most ? k : most);
}
__host__ __device__ __forceinline__ int fq_parts(int64_t n) { return n <= 0 ? 0 : fq_spread(n, kFqPartMin, kFqParts); }
__host__ __device__ __forceinline__ int fq_appliers(int64_t n) { return n <= 0 ? 1 : fq_spread(n, kFqApplyMin, kFqApply); }

// min / max over the finite elements of this lane's share (t0, t0 + stride, ... in float4 units when x is 16-byte aligned)
__device__ __forceinline__ void minmax_span(const float *__restrict__ x, int64_t n, int64_t t0, int64_t stride, float *mn_out, float *mx_out) {
    float mn = INFINITY, mx = -INFINITY;
    auto take = [&](float v) {
        if (isfinite(v)) {
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    };
    int64_t head = 0;
    if (((uintptr_t)x & 15) == 0) {
        const float4 *x4 = (const float4 *)x;
        const int64_t n4 = n >> 2;
        int64_t j = t0;
        for (; j + 3 * stride < n4; j += 4 * stride) {   // four loads in flight per lane
            const float4 a = x4[j], b = x4[j + stride], c = x4[j + 2 * stride], d = x4[j + 3 * stride];
            take(a.x); take(a.y); take(a.z); take(a.w);
            take(b.x); take(b.y); take(b.z); take(b.w);
            take(c.x); take(c.y); take(c.z); take(c.w);
            take(d.x); take(d.y); take(d.z); take(d.w);
        }
        for (; j < n4; j += stride) {
            const float4 a = x4[j];
            take(a.x); take(a.y); take(a.z); take(a.w);
        }
        head = n4 << 2;
    }
    for (int64_t i = head + t0; i < n; i += stride) take(x[i]);
    *mn_out = mn;
    *mx_out = mx;
}

// y = f(x) elementwise over this lane's share, float4 loads / stores when both are 16-byte aligned
template <class F>
__device__ __forceinline__ void map_span(const float *__restrict__ x, float *__restrict__ y, int64_t n, int64_t t0, int64_t stride, F f) {
    int64_t head = 0;
    if ((((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
        const float4 *x4 = (const float4 *)x;
        float4 *y4 = (float4 *)y;
        const int64_t n4 = n >> 2;
        int64_t j = t0;
        for (; j + stride < n4; j += 2 * stride) {   // two loads in flight per lane (four measured no faster: the pass is half ALU)
            float4 a = x4[j], b = x4[j + stride];
            a.x = f(a.x); a.y = f(a.y); a.z = f(a.z); a.w = f(a.w);
            b.x = f(b.x); b.y = f(b.y); b.z = f(b.z); b.w = f(b.w);
            y4[j] = a;
            y4[j + stride] = b;
        }
        for (; j < n4; j += stride) {
            float4 a = x4[j];
            a.x = f(a.x); a.y = f(a.y); a.z = f(a.z); a.w = f(a.w);
            y4[j] = a;
        }
        head = n4 << 2;
    }
    for (int64_t i = head + t0; i < n; i += stride) y[i] = f(x[i]);
}

// every lane of the workgroup leaves with the workgroup's min / max (s: 8 floats of LDS; the trailing barrier frees it for the next call)
__device__ __forceinline__ void block_minmax(float *mn, float *mx, float *s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        *mn = fminf(*mn, __shfl_xor(*mn, off, 64));
        *mx = fmaxf(*mx, __shfl_xor(*mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s[threadIdx.x >> 6] = *mn;
        s[4 + (threadIdx.x >> 6)] = *mx;
    }
    __syncthreads();
    *mn = fminf(fminf(s[0], s[1]), fminf(s[2], s[3]));
    *mx = fmaxf(fmaxf(s[4], s[5]), fmaxf(s[6], s[7]));
    __syncthreads();
}

// the fold of a tensor's nb partials {min, max} (the applying workgroups each do it: no third launch, no cross-workgroup hand-off)
__device__ __forceinline__ void fold_parts(const float *__restrict__ part, int nb, float *mn, float *mx, float *s) {
    float a = INFINITY, b = -INFINITY;
    for (int k = threadIdx.x; k < nb; k += kFqThreads) {
        a = fminf(a, part[2 * k]);
        b = fmaxf(b, part[2 * k + 1]);
    }
    block_minmax(&a, &b, s);
    *mn = a;
    *mx = b;
}

__device__ __forceinline__ float f16_round_trip(float v) { return f16_bits_to_f32(f32_to_f16_bits(v)); }

// ---- weights: a list of tensors ----
// Tensor `it` takes workgroups off_it, off_it + 1, ... (mod the grid) with off_it = the workgroups the tensors before it took: the small
// tensors of a model land on different workgroups and run side by side instead of queueing behind each other on the first few.
__global__ __launch_bounds__(kFqThreads) void fq_minmax_multi_kernel(const th_fq_item *__restrict__ items, int n_items, float *__restrict__ part) {
    __shared__ float s[8];
    int off = 0;
    for (int it = 0; it < n_items; ++it) {
        const th_fq_item t = items[it];
        const int nb = t.qtype == TH_QTYPE_INT8 ? fq_parts(t.n) : 0;
        const int lb = ((int)blockIdx.x - off + kFqParts) % kFqParts;   // this workgroup's rank for the tensor
        off = (off + nb) % kFqParts;
        if (lb >= nb) continue;   // (uniform over the workgroup)
        float mn, mx;
        minmax_span(t.d_x, t.n, (int64_t)lb * kFqThreads + threadIdx.x, (int64_t)nb * kFqThreads, &mn, &mx);
        block_minmax(&mn, &mx, s);
        if (threadIdx.x == 0) {
            float *p = part + ((size_t)it * kFqParts + lb) * 2;
            p[0] = mn;
            p[1] = mx;
        }
    }
}

__global__ __launch_bounds__(kFqThreads) void fq_apply_multi_kernel(const th_fq_item *__restrict__ items, int n_items, const float *__restrict__ part) {
    __shared__ float s[8];
    int off = 0;
    for (int it = 0; it < n_items; ++it) {
        const th_fq_item t = items[it];
        const int na = fq_appliers(t.n);
        const int lb = ((int)blockIdx.x - off + kFqApply) % kFqApply;
        off = (off + na) % kFqApply;
        if (lb >= na) continue;   // (uniform; rank 0 always applies: it writes the pair)
        const int64_t t0 = (int64_t)lb * kFqThreads + threadIdx.x, stride = (int64_t)na * kFqThreads;
        if (t.qtype == TH_QTYPE_INT8) {
            float mn, mx, min_val, scale;
            fold_parts(part + (size_t)it * kFqParts * 2, fq_parts(t.n), &mn, &mx, s);
            int8_params(mn, mx, &min_val, &scale);
            if (lb == 0 && threadIdx.x == 0 && t.d_params) {
                t.d_params[0] = min_val;
                t.d_params[1] = scale;
            }
            map_span(t.d_x, t.d_y, t.n, t0, stride, [=](float v) { return dequant_int8(quant_int8(v, min_val, scale), scale, min_val); });
        } else {
            map_span(t.d_x, t.d_y, t.n, t0, stride, [](float v) { return f16_round_trip(v); });
        }
    }
}

// ---- activations: one tensor ----
__global__ __launch_bounds__(kFqThreads) void fq_act_minmax_kernel(const float *__restrict__ x, int64_t n, float *__restrict__ part) {
    __shared__ float s[8];
    float mn, mx;
    minmax_span(x, n, (int64_t)blockIdx.x * kFqThreads + threadIdx.x, (int64_t)gridDim.x * kFqThreads, &mn, &mx);
    block_minmax(&mn, &mx, s);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = mn;
        part[2 * blockIdx.x + 1] = mx;
    }
}

// symmetric int8 (fake_quantize.rs:71-82 with zero_point 0, 155-162): scale = max(|min|, |max|) / 127 over the finite min / max with the
// reference's edge cases (94-118: all zero -> (0, 1), all equal to m -> (0.9 m, 1.1 m)); y = clamp(round(x / scale) as i32, -128, 127) * scale
__global__ __launch_bounds__(kFqThreads) void fq_act_int8_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t n,
                                                                const float *__restrict__ part, int nb, float *__restrict__ d_scale) {
    __shared__ float s[8];
    float mn, mx;
    fold_parts(part, nb, &mn, &mx, s);
    if (mn == mx) {
        if (mn == 0.0f) {
            mn = 0.0f;
            mx = 1.0f;
        } else {
            const float m = mn;
            mn = m * 0.9f;
            mx = m * 1.1f;
        }
    }
    const float scale = fmaxf(fabsf(mn), fabsf(mx)) / 127.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0 && d_scale) d_scale[0] = scale;
    map_span(x, y, n, (int64_t)blockIdx.x * kFqThreads + threadIdx.x, (int64_t)gridDim.x * kFqThreads, [=](float v) {
        const int q = rust_f32_as_i32(roundf(v / scale));
        return (float)(q < -128 ? -128 : (q > 127 ? 127 : q)) * scale;
    });
}

__global__ __launch_bounds__(kFqThreads) void fq_act_f16_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t n, float *__restrict__ d_scale) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && d_scale) d_scale[0] = 0.0f;   // (a half round trip has no scale)
    map_span(x, y, n, (int64_t)blockIdx.x * kFqThreads + threadIdx.x, (int64_t)gridDim.x * kFqThreads, [](float v) { return f16_round_trip(v); });
}

}  // namespace th

using namespace th;

extern "C" {

int th_fake_quant_multi(th_ctx *ctx, const th_fq_item *d_items, int n_items) {
    TH_REQUIRE(ctx && n_items >= 0 && (n_items == 0 || d_items), "th_fake_quant_multi: null argument or negative count");
    if (n_items == 0) return 0;
    void *part = nullptr;
    if (th_malloc(ctx, (size_t)n_items * kFqParts * 2 * sizeof(float), &part)) return 1;
    hipLaunchKernelGGL(fq_minmax_multi_kernel, dim3(kFqParts), dim3(kFqThreads), 0, ctx->stream, d_items, n_items, (float *)part);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(fq_apply_multi_kernel, dim3(kFqApply), dim3(kFqThreads), 0, ctx->stream, d_items, n_items, (const float *)part);
    TH_LAUNCH_CHECK();
    return th_free(ctx, part);
}

int th_fake_quant_act(th_ctx *ctx, const float *d_x, float *d_y, int64_t n, int qtype, float *d_scale) {
    TH_REQUIRE(ctx && n >= 0 && (n == 0 || (d_x && d_y)), "th_fake_quant_act: null argument");
    TH_REQUIRE(qtype == TH_QTYPE_INT8 || qtype == TH_QTYPE_F16, "th_fake_quant_act: qtype %d is neither TH_QTYPE_INT8 nor TH_QTYPE_F16", qtype);
    if (qtype == TH_QTYPE_F16) {
        hipLaunchKernelGGL(fq_act_f16_kernel, dim3(fq_appliers(n)), dim3(kFqThreads), 0, ctx->stream, d_x, d_y, n, d_scale);
        TH_LAUNCH_CHECK();
        return 0;
    }
    const int nb = std::max(fq_parts(n), 1);
    void *part = nullptr;
    if (th_malloc(ctx, (size_t)nb * 2 * sizeof(float), &part)) return 1;
    hipLaunchKernelGGL(fq_act_minmax_kernel, dim3(nb), dim3(kFqThreads), 0, ctx->stream, d_x, n, (float *)part);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(fq_act_int8_kernel, dim3(fq_appliers(n)), dim3(kFqThreads), 0, ctx->stream, d_x, d_y, n, (const float *)part, nb, d_scale);
    TH_LAUNCH_CHECK();
    return th_free(ctx, part);
}

}  // extern "C"
