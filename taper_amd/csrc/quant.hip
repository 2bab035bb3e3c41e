// quant.hip -- the reference's post-training-quantization STORAGE codecs that do real work (src/tensor.rs:2110-2288;
// Int4 / BFloat16 / NF4 are placeholders there): int8 affine quantisation over the finite min / max of the tensor, and the
// hand-rolled IEEE half conversion.  Integer / bit work: restated literally (including the half-up rounding whose mantissa
// carry is OR-ed, not added, into the exponent field) and held to bit-exact parity.  HBM-bound, one pass each.
#include "common.h"
#include "quant_dev.h"

namespace th {

__global__ __launch_bounds__(256) void f32_to_f16_kernel(const float *__restrict__ x, uint16_t *__restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = f32_to_f16_bits(x[i]);
}
__global__ __launch_bounds__(256) void f16_to_f32_kernel(const uint16_t *__restrict__ x, float *__restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] = f16_bits_to_f32(x[i]);
}

// finite min / max (tensor.rs:2117-2125): per-block partials, then one block folds them; min / max are order-independent
__global__ __launch_bounds__(256) void minmax_finite_kernel(const float *__restrict__ x, size_t n, float *__restrict__ part) {
    __shared__ float smin[4], smax[4];
    float mn = INFINITY, mx = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = x[i];
        if (isfinite(v)) {
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_down(mn, off, 64));
        mx = fmaxf(mx, __shfl_down(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = mn;
        smax[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        part[2 * blockIdx.x + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

// params = {min_val, scale} (tensor.rs:2127-2134), then q = round((x - min) / scale) as i32 + qmin, clamped (2136-2143)
__global__ __launch_bounds__(256) void int8_params_kernel(const float *__restrict__ part, int n_part, float *__restrict__ params) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < n_part; ++i) {
        mn = fminf(mn, part[2 * i]);
        mx = fmaxf(mx, part[2 * i + 1]);
    }
    int8_params(mn, mx, &params[0], &params[1]);
}

__global__ __launch_bounds__(256) void quantize_int8_kernel(const float *__restrict__ x, int8_t *__restrict__ q, size_t n,
                                                            const float *__restrict__ params) {
    const float mn = params[0], scale = params[1];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        q[i] = (int8_t)quant_int8(x[i], mn, scale);
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
    const int blocks = n == 0 ? 1 : (int)std::min<size_t>(1024, (n + 255) / 256);
    void *part = nullptr;
    if (th_malloc(ctx, (size_t)blocks * 2 * sizeof(float), &part)) return 1;
    hipLaunchKernelGGL(minmax_finite_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_x, n, (float *)part);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(int8_params_kernel, dim3(1), dim3(64), 0, ctx->stream, (const float *)part, blocks, d_params);
    TH_LAUNCH_CHECK();
    if (n) {
        hipLaunchKernelGGL(quantize_int8_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, ctx->stream, d_x, d_q, n, (const float *)d_params);
        TH_LAUNCH_CHECK();
    }
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
