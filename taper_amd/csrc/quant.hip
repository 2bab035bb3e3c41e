// quant.hip -- the reference's post-training-quantization STORAGE codecs that do real work (src/tensor.rs:2110-2288;
// Int4 / BFloat16 / NF4 are placeholders there): int8 affine quantisation over the finite min / max of the tensor, and the
// hand-rolled IEEE half conversion.  Integer / bit work: restated literally (including the half-up rounding whose mantissa
// carry is OR-ed, not added, into the exponent field) and held to bit-exact parity.  HBM-bound, one pass each.
// Also here: a frozen BatchNorm2d for the quantized twins -- th_fold_batchnorm2d makes {a, b} per channel and
// th_channel_affine_fwd is the layer where no static conv's epilogue takes it.
#include "common.h"
#include "quant_dev.h"
#include "stream_dev.h"

#include <cmath>

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

// ---- one pair per channel ----
// Rows: channel c is len consecutive floats.  A workgroup per channel, lanes along the row: the min / max walk (stream_dev.h's span, from
// the row's own address), the workgroup fold, then the codes -- the row's second read comes from the cache.  One launch.
__global__ __launch_bounds__(kStreamThreads) void quantize_int8_rows_kernel(const float *__restrict__ x, int8_t *__restrict__ q, int channels, int64_t len,
                                                                            float *__restrict__ params) {
    __shared__ float s[8];
    for (int64_t c = blockIdx.x; c < channels; c += gridDim.x) {
        const float *xr = x + (size_t)c * len;
        int8_t *qr = q + (size_t)c * len;
        float mn, mx, min_val, scale;
        minmax_span<MinMaxFinite, true>(xr, xr, len, threadIdx.x, kStreamThreads, &mn, &mx);
        block_minmax(&mn, &mx, s);
        int8_params(mn, mx, &min_val, &scale);
        if (threadIdx.x == 0) {
            params[2 * c] = min_val;
            params[2 * c + 1] = scale;
        }
        for (int64_t i = threadIdx.x; i < len; i += kStreamThreads) qr[i] = (int8_t)quant_int8(xr[i], min_val, scale);
    }
}

// Columns: element k of channel c lies at x[k channels + c].  Lane = channel, so a wave reads 64 consecutive floats; workgroup
// (bx, by) owns channels 64 bx .. + 63 and its wave v the elements k = 4 by + v, + 4 gridDim.y, ...: the K walk is split over waves and
// workgroups.  The first pass leaves part[by][c] = {min, max} of a workgroup's share; the second folds a channel's gridDim.y partials
// (compares: any order gives the same bits), writes the pair and codes the same share.
constexpr int kQuantColSplit = 32;   // workgroups along K at most, 16 elements of every channel each at least

__device__ __forceinline__ void cols_fold(float *mn, float *mx, float (*s)[4][64], int lane, int wave) {   // the four waves' values of a channel
    s[0][wave][lane] = *mn;
    s[1][wave][lane] = *mx;
    __syncthreads();
    *mn = fminf(fminf(s[0][0][lane], s[0][1][lane]), fminf(s[0][2][lane], s[0][3][lane]));
    *mx = fmaxf(fmaxf(s[1][0][lane], s[1][1][lane]), fmaxf(s[1][2][lane], s[1][3][lane]));
}

__global__ __launch_bounds__(256) void minmax_cols_kernel(const float *__restrict__ x, int channels, int64_t len, float *__restrict__ part) {
    __shared__ float s[2][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    float mn = INFINITY, mx = -INFINITY;
    if (c < channels)
        for (int64_t k = blockIdx.y * 4 + wave; k < len; k += 4 * gridDim.y) {
            const float v = x[(size_t)k * channels + c];
            MinMaxFinite::take(mn, mx, v, v);
        }
    cols_fold(&mn, &mx, s, lane, wave);
    if (wave == 0 && c < channels) {
        part[((size_t)blockIdx.y * channels + c) * 2] = mn;
        part[((size_t)blockIdx.y * channels + c) * 2 + 1] = mx;
    }
}

__global__ __launch_bounds__(256) void quantize_int8_cols_kernel(const float *__restrict__ x, int8_t *__restrict__ q, int channels, int64_t len,
                                                                 const float *__restrict__ part, float *__restrict__ params) {
    __shared__ float s[2][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    float mn = INFINITY, mx = -INFINITY, min_val, scale;
    if (c < channels)
        for (int p = wave; p < (int)gridDim.y; p += 4) {
            mn = fminf(mn, part[((size_t)p * channels + c) * 2]);
            mx = fmaxf(mx, part[((size_t)p * channels + c) * 2 + 1]);
        }
    cols_fold(&mn, &mx, s, lane, wave);
    if (c >= channels) return;
    int8_params(mn, mx, &min_val, &scale);
    if (blockIdx.y == 0 && wave == 0) {
        params[2 * c] = min_val;
        params[2 * c + 1] = scale;
    }
    for (int64_t k = blockIdx.y * 4 + wave; k < len; k += 4 * gridDim.y) q[(size_t)k * channels + c] = (int8_t)quant_int8(x[(size_t)k * channels + c], min_val, scale);
}

__global__ __launch_bounds__(256) void dequantize_int8_kernel(const int8_t *__restrict__ q, float *__restrict__ y, size_t n, float scale,
                                                              int zero_point, float min_val) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        y[i] = (float)((int)q[i] - zero_point) * scale + min_val;                     // tensor.rs:357 (two roundings: contraction is off)
}

// ---- a frozen BatchNorm2d ----
// The fold: {a, b} of every channel from the layer's parameters and its running pair; a lane a channel, every operation rounded once.
// invstd is batchnorm.hip's eval expression with sqrtf in the place of __fsqrt_rn: the intrinsic is the hardware's square root, good to
// one ulp, where sqrtf rounds correctly -- a snapshot that a numpy restatement gives bit for bit needs the latter.
__global__ __launch_bounds__(kStreamThreads) void batchnorm_fold_kernel(const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                        const float *__restrict__ running_mean, const float *__restrict__ running_var,
                                                                        float eps, int c, float *__restrict__ affine) {
    for (int64_t ch = grid_t0(); ch < c; ch += grid_stride()) {
        const float invstd = __fdiv_rn(1.0f, sqrtf(running_var[ch] + eps));
        const float a = __fmul_rn(gamma[ch], invstd);
        affine[2 * ch] = a;
        affine[2 * ch + 1] = __fsub_rn(beta[ch], __fmul_rn(running_mean[ch], a));
    }
}

// The standalone layer over NCHW: the tensor is one stream of `units` units of V (float4s when hw % 4 == 0 and both pointers are 16-byte
// aligned, then no unit straddles a plane; floats otherwise), upp of them a plane.  A lane walks t0, t0 + stride, ... and keeps its place
// {offset in the plane, channel} by additions: one 64-bit division a lane, before the walk.
template <class V>
__global__ __launch_bounds__(kStreamThreads) void channel_affine_kernel(const float *__restrict__ x, const float *__restrict__ affine, int64_t units, int upp,
                                                                        int c, int relu, float *__restrict__ y) {
    const int64_t stride = grid_stride();
    int64_t j = grid_t0();
    if (j >= units) return;
    const int64_t plane = j / upp, dplane = stride / upp;
    int off = (int)(j - plane * upp), ch = (int)(plane % c);
    const int doff = (int)(stride - dplane * upp), dch = (int)(dplane % c);
#pragma unroll 2
    for (; j < units; j += stride) {
        const float a = affine[2 * ch], b = affine[2 * ch + 1];
        put(y, j, vmap([=](float v) { return affine_value(v, a, b, relu); }, at<V>(x, j)));
        off += doff;
        ch += dch;
        if (off >= upp) {   // (off < 2 upp and ch <= 2 c - 1 here: one step back each)
            off -= upp;
            ++ch;
        }
        if (ch >= c) ch -= c;
    }
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

// th_quantize_int8, and th_quantize_int8_channels' single channel (fn: the caller's name for the message)
static int quantize_int8_run(const char *fn, th_ctx *ctx, const float *d_x, int8_t *d_q, size_t n, float *d_params) {
    TH_REQUIRE(ctx && d_params && (n == 0 || (d_x && d_q)), "%s: null argument", fn);
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

int th_quantize_int8(th_ctx *ctx, const float *d_x, int8_t *d_q, size_t n, float *d_params) {
    return quantize_int8_run("th_quantize_int8", ctx, d_x, d_q, n, d_params);
}

int th_quantize_int8_channels(th_ctx *ctx, const float *d_x, int channels, int64_t len, int64_t chan_stride, int64_t elem_stride, int8_t *d_q,
                              float *d_params) {
    TH_REQUIRE(ctx && d_x && d_q && d_params, "th_quantize_int8_channels: null argument");
    TH_REQUIRE(channels >= 1 && len >= 1, "th_quantize_int8_channels: channels=%d or len=%lld below 1", channels, (long long)len);
    const bool rows = elem_stride == 1 && (chan_stride == len || channels == 1), cols = chan_stride == 1 && elem_stride == channels;
    TH_REQUIRE(rows || cols,
               "th_quantize_int8_channels: chan_stride=%lld elem_stride=%lld is neither rows (chan_stride == len, elem_stride == 1) nor columns "
               "(chan_stride == 1, elem_stride == channels)",
               (long long)chan_stride, (long long)elem_stride);
    if (rows && channels == 1) return quantize_int8_run("th_quantize_int8_channels", ctx, d_x, d_q, (size_t)len, d_params);
    if (rows) {
        hipLaunchKernelGGL(quantize_int8_rows_kernel, dim3(std::min(channels, kNumCU * 32)), dim3(kStreamThreads), 0, ctx->stream, d_x, d_q, channels, len, d_params);
        TH_LAUNCH_CHECK();
        return 0;
    }
    const dim3 grid(ceil_div(channels, 64), stream_grid(len, 16, kQuantColSplit));
    void *part = nullptr;
    if (th_malloc(ctx, (size_t)grid.y * channels * 2 * sizeof(float), &part)) return 1;
    hipLaunchKernelGGL(minmax_cols_kernel, grid, dim3(256), 0, ctx->stream, d_x, channels, len, (float *)part);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(quantize_int8_cols_kernel, grid, dim3(256), 0, ctx->stream, d_x, d_q, channels, len, (const float *)part, d_params);
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

int th_fold_batchnorm2d(th_ctx *ctx, const float *d_gamma, const float *d_beta, const float *d_running_mean, const float *d_running_var, float eps, int c,
                        float *d_affine) {
    TH_REQUIRE(ctx && d_gamma && d_beta && d_running_mean && d_running_var && d_affine, "th_fold_batchnorm2d: null argument");
    TH_REQUIRE(c > 0, "th_fold_batchnorm2d: c must be positive (got %d)", c);
    TH_REQUIRE(std::isfinite(eps) && eps > 0.0f, "th_fold_batchnorm2d: eps must be finite and positive (got %g)", (double)eps);
    hipLaunchKernelGGL(batchnorm_fold_kernel, dim3(stream_grid(c, kStreamThreads, kNumCU)), dim3(kStreamThreads), 0, ctx->stream, d_gamma, d_beta, d_running_mean,
                       d_running_var, eps, c, d_affine);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_channel_affine_fwd(th_ctx *ctx, const float *d_x, const float *d_affine, int n, int c, int hw, int relu, float *d_y) {
    TH_REQUIRE(ctx && d_x && d_affine && d_y, "th_channel_affine_fwd: null argument");
    TH_REQUIRE(n >= 0 && c > 0 && hw > 0, "th_channel_affine_fwd: c and hw must be positive, n not negative (got n=%d c=%d hw=%d)", n, c, hw);
    TH_REQUIRE((int64_t)n * hw < ((int64_t)1 << 31), "th_channel_affine_fwd: %lld elements per channel: fewer than 2^31 are supported", (long long)n * hw);
    if (n == 0) return 0;
    const bool wide = hw % 4 == 0 && (((uintptr_t)d_x | (uintptr_t)d_y) & 15) == 0;
    const int upp = wide ? hw / 4 : hw;
    const int64_t units = (int64_t)n * c * upp;
    const dim3 grid(stream_grid(units, 2 * kStreamThreads, kNumCU * 8));   // two units a lane at least
    hipLaunchKernelGGL(wide ? channel_affine_kernel<float4> : channel_affine_kernel<float>, grid, dim3(kStreamThreads), 0, ctx->stream, d_x, d_affine, units, upp, c,
                       relu, d_y);
    TH_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
