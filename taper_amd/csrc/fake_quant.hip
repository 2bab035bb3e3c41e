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
// The span walk, the finite-only min / max partials and their fold are stream_dev.h's: th_quantize_int8 launches the same partials kernel.
#include "common.h"
#include "quant_dev.h"
#include "stream_dev.h"

namespace th {

constexpr int kFqThreads = kStreamThreads;
constexpr int kFqParts = 512;                   // workgroups of the min / max pass (2 per CU): the most partials a tensor leaves
constexpr int kFqApply = 1024;                  // workgroups of the applying pass (4 per CU)
constexpr int64_t kFqPartMin = 4 * 256 * 8;     // elements per min / max workgroup at least (8 float4 loads per lane)
constexpr int64_t kFqApplyMin = 4 * 256;        // ... per applying workgroup (one float4 per lane)

__host__ __device__ __forceinline__ int fq_parts(int64_t n) { return n <= 0 ? 0 : stream_grid(n, kFqPartMin, kFqParts); }
__host__ __device__ __forceinline__ int fq_appliers(int64_t n) { return n <= 0 ? 1 : stream_grid(n, kFqApplyMin, kFqApply); }

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
        minmax_span<MinMaxFinite, true>(t.d_x, t.d_x, t.n, (int64_t)lb * kFqThreads + threadIdx.x, (int64_t)nb * kFqThreads, &mn, &mx);
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
    map_span(x, y, n, grid_t0(), grid_stride(), [=](float v) {
        const int q = rust_f32_as_i32(roundf(v / scale));
        return (float)(q < -128 ? -128 : (q > 127 ? 127 : q)) * scale;
    });
}

__global__ __launch_bounds__(kFqThreads) void fq_act_f16_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t n, float *__restrict__ d_scale) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && d_scale) d_scale[0] = 0.0f;   // (a half round trip has no scale)
    map_span(x, y, n, grid_t0(), grid_stride(), [](float v) { return f16_round_trip(v); });
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
    hipLaunchKernelGGL((minmax_parts_kernel<MinMaxFinite, true>), dim3(nb), dim3(kFqThreads), 0, ctx->stream, d_x, d_x, n, (float *)part);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(fq_act_int8_kernel, dim3(fq_appliers(n)), dim3(kFqThreads), 0, ctx->stream, d_x, d_y, n, (const float *)part, nb, d_scale);
    TH_LAUNCH_CHECK();
    return th_free(ctx, part);
}

}  // extern "C"
