// quant.hip -- the reference's post-training-quantization STORAGE codecs that do real work (src/tensor.rs:2110-2288;
// Int4 / BFloat16 / NF4 are placeholders there): int8 affine quantisation over the finite min / max of the tensor, and the
// hand-rolled IEEE half conversion.  Integer / bit work: restated literally (including the half-up rounding whose mantissa
// carry is OR-ed, not added, into the exponent field) and held to bit-exact parity.  HBM-bound, one pass each.
#include "common.h"
#include "quant_dev.h"
#include "stream_dev.h"

namespace th {

__global__ __launch_bounds__(256) void f32_to_f16_kernel(const float *__restrict__ x, uint16_t *__restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = f32_to_f16_bits(x[i]);
}
__global__ __launch_bounds__(256) void f16_to_f32_kernel(const uint16_t *__restrict__ x, float *__restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = f16_bits_to_f32(x[i]);
}

// int8 affine over the finite min / max (stream_dev.h's MinMaxFinite partials, folded by every workgroup here as fq_act_int8_kernel does):
// params = {min_val, scale} (tensor.rs:2127-2134), then q = round((x - min) / scale) as i32 + qmin, clamped (2136-2143)
constexpr int kQuantParts = 1024;   // workgroups of the min / max pass at most, 256 elements each at least

__global__ __launch_bounds__(256) void quantize_int8_kernel(const float *__restrict__ x, int8_t *__restrict__ q, size_t n,
                                                            const float *__restrict__ part, int nb, float *__restrict__ params) {
    __shared__ float s[8];
    float mn, mx, min_val, scale;
    fold_parts(part, nb, &mn, &mx, s);   // (no partials for n == 0: +inf / -inf, as the empty fold always left them)
    int8_params(mn, mx, &min_val, &scale);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        params[0] = min_val;
        params[1] = scale;
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        q[i] = (int8_t)quant_int8(x[i], min_val, scale);
    }
}

__global__ __launch_bounds__(256) void dequantize_int8_kernel(const int8_t *__restrict__ q, float *__restrict__ y, size_t n, float scale,
                                                              int zero_point, float min_val) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        y[i] = (float)((int)q[i] - zero_point) * scale + min_val;                     // tensor.rs:357 (two roundings: contraction is off)
}

}  // namespace th

using namespace th;

extern "C" {

int th_f32_to_f16(th_ctx *ctx, const float *d_x, uint16_t *d_y, size_t n) {
    TH_REQUIRE(ctx && (n == 0 || (d_x && d_y)), "th_f32_to_f16: null argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, ctx->stream, d_x, d_y, n);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_f16_to_f32(th_ctx *ctx, const uint16_t *d_x, float *d_y, size_t n) {
    TH_REQUIRE(ctx && (n == 0 || (d_x && d_y)), "th_f16_to_f32: null argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, ctx->stream, d_x, d_y, n);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_quantize_int8(th_ctx *ctx, const float *d_x, int8_t *d_q, size_t n, float *d_params) {
    TH_REQUIRE(ctx && d_params && (n == 0 || (d_x && d_q)), "th_quantize_int8: null argument");
    const int nb = n == 0 ? 0 : stream_grid((int64_t)n, 256, kQuantParts);
    void *part = nullptr;
    if (th_malloc(ctx, (size_t)std::max(nb, 1) * 2 * sizeof(float), &part)) return 1;
    if (nb) {
        hipLaunchKernelGGL((minmax_parts_kernel<MinMaxFinite, true>), dim3(nb), dim3(256), 0, ctx->stream, d_x, d_x, (int64_t)n, (float *)part);
        TH_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(quantize_int8_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, ctx->stream, d_x, d_q, n, (const float *)part, nb, d_params);
    TH_LAUNCH_CHECK();
    return th_free(ctx, part);
}

int th_dequantize_int8(th_ctx *ctx, const int8_t *d_q, float *d_y, size_t n, float scale, int zero_point, float min_val) {
    TH_REQUIRE(ctx && (n == 0 || (d_q && d_y)), "th_dequantize_int8: null argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(dequantize_int8_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, ctx->stream, d_q, d_y, n, scale, zero_point, min_val);
    TH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
