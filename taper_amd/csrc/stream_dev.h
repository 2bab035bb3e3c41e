// stream_dev.h -- the building blocks the quantization kernels share (quant.hip, fake_quant.hip, observers.hip), once each: the walk of
// a lane's share of an HBM stream in 16-byte pieces, the workgroup min / max, the two min / max policies, the per-workgroup {min, max}
// partials of a tensor and their fold, and the grid size of such a pass.  Min / max are exact, so every grouping and every order of a
// fold gives the same bits: fake quantization trains against the bits quantize() packs because both take their min / max from here.
#pragma once
#include "common.h"
#include <utility>

namespace th {

constexpr int kStreamThreads = 256;   // lanes of every workgroup here: block_minmax folds four waves

// workgroups for n > 0 elements: at least `per` elements each, at most `most` of them
__host__ __device__ __forceinline__ int stream_grid(int64_t n, int64_t per, int most) {
    const int64_t k = (n + per - 1) / per;
    return (int)(k < most ? k : most);
}

// a lane's first index and the step of a pass that gives the whole grid one tensor
__device__ __forceinline__ int64_t grid_t0() { return (int64_t)blockIdx.x * kStreamThreads + threadIdx.x; }
__device__ __forceinline__ int64_t grid_stride() { return (int64_t)gridDim.x * kStreamThreads; }

__device__ __forceinline__ bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// element j of p seen as an array of V (float or float4)
template <class V> __device__ __forceinline__ V &at(float *p, int64_t j) { return ((V *)p)[j]; }
template <class V> __device__ __forceinline__ const V &at(const float *p, int64_t j) { return ((const V *)p)[j]; }
template <class V> __device__ __forceinline__ void put(float *p, int64_t j, const V &v) { at<V>(p, j) = v; }

// f over floats, or over each component of float4s
template <class F, class... A> __device__ __forceinline__ float vmap(F f, float a0, A... a) { return f(a0, a...); }
template <class F, class... A> __device__ __forceinline__ float4 vmap(F f, float4 a0, A... a) {
    return make_float4(f(a0.x, a.x...), f(a0.y, a.y...), f(a0.z, a.z...), f(a0.w, a.w...));
}

// ---- the span walk ----
// This lane's share t0, t0 + stride, ... of [0, n) of the input streams `in`: with 16-byte aligned pointers (the caller says, its
// outputs included) in float4 units, kFlight trips at a time with all their loads -- stream by stream -- issued before the first is
// used, then single float4s, then the scalar tail; otherwise all of it by scalars.  use(j, a, b, ...) gets element j of every stream
// (float4s or floats, by reference) and does the rest: a reduction, or put(out, j, ...).
// A trip's values are copy-initialised straight from memory into one flat array, v[stream * kFlight + trip], and handed on by reference:
// a float4 that passes through a by-value return or argument reaches the optimiser split in two halves, and the kernels came out
// with other registers and another schedule than the hand-written loops this replaces.
template <int kFlight, int K, class Use, int... S>
__device__ __forceinline__ void span_use(Use &use, int64_t j, const float4 *v, std::integer_sequence<int, S...>) {
    use(j, v[S * kFlight + K]...);
}
template <class Use, int... K, int... I, class... In>   // I = 0 .. streams * kFlight
__device__ __forceinline__ void span_trips(int64_t j, int64_t stride, Use &use, std::integer_sequence<int, K...>, std::integer_sequence<int, I...>, In... in) {
    constexpr int kFlight = sizeof...(K);
    const float *const p[] = {in...};
    const float4 v[] = {at<float4>(p[I / kFlight], j + (I % kFlight) * stride)...};
    (span_use<kFlight, K>(use, j + K * stride, v, std::make_integer_sequence<int, sizeof...(In)>()), ...);
}
template <int kFlight, class Use, class... In>
__device__ __forceinline__ void span_walk(bool aligned, int64_t n, int64_t t0, int64_t stride, Use use, In... in) {
    int64_t head = 0;
    if (aligned) {
        const int64_t n4 = n >> 2;
        int64_t j = t0;
        for (; j + (kFlight - 1) * stride < n4; j += kFlight * stride)
            span_trips(j, stride, use, std::make_integer_sequence<int, kFlight>(), std::make_integer_sequence<int, kFlight * sizeof...(In)>(), in...);
        for (; j < n4; j += stride) use(j, at<float4>(in, j)...);
        head = n4 << 2;
    }
    for (int64_t i = head + t0; i < n; i += stride) use(i, at<float>(in, i)...);
}

// y = f(x) elementwise; two loads in flight per lane (four measured no faster: the pass is half ALU)
template <class F>
__device__ __forceinline__ void map_span(const float *__restrict__ x, float *__restrict__ y, int64_t n, int64_t t0, int64_t stride, F f) {
    span_walk<2>(aligned16(x, y), n, t0, stride, [=](int64_t j, const auto &a) { put(y, j, vmap(f, a)); }, x);
}

// ---- min / max ----
// The two policies differ in what an infinity does, and in nothing else.
// Finite only (tensor.rs:2117-2125 for quantize(), fake_quantize.rs:94-118 for fake quantization): NaNs and infinities are skipped.
struct MinMaxFinite {
    static __device__ __forceinline__ void take(float &mn, float &mx, float p, float q) {
        if (isfinite(p)) mn = fminf(mn, p);
        if (isfinite(q)) mx = fmaxf(mx, q);
    }
};
// NaN-ignoring (observers.rs' global_min / global_max and the histogram's first range: folds of f32::min / f32::max from +inf / -inf):
// a NaN operand loses to a number (fminf / fmaxf), an infinity takes part.
struct MinMaxNanIgnoring {
    static __device__ __forceinline__ void take(float &mn, float &mx, float p, float q) {
        mn = fminf(mn, p);
        mx = fmaxf(mx, q);
    }
};
template <class Policy> __device__ __forceinline__ void minmax_take(float &mn, float &mx, const float &p, const float &q) { Policy::take(mn, mx, p, q); }
template <class Policy> __device__ __forceinline__ void minmax_take(float &mn, float &mx, const float4 &p, const float4 &q) {
    Policy::take(mn, mx, p.x, q.x);
    Policy::take(mn, mx, p.y, q.y);
    Policy::take(mn, mx, p.z, q.z);
    Policy::take(mn, mx, p.w, q.w);
}

// min over a and max over b of this lane's share, from +inf / -inf (kSame: a == b, one read); four (eight) loads in flight per lane
template <class Policy, bool kSame>
__device__ __forceinline__ void minmax_span(const float *__restrict__ a, const float *__restrict__ b, int64_t n, int64_t t0, int64_t stride,
                                            float *mn_out, float *mx_out) {
    float mn = INFINITY, mx = -INFINITY;
    if (kSame) b = a;   // (the second load of an element folds into the first)
    span_walk<4>(aligned16(a, b), n, t0, stride, [&](int64_t, const auto &p, const auto &q) { minmax_take<Policy>(mn, mx, p, q); }, a, b);
    *mn_out = mn;
    *mx_out = mx;
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

// the first pass: workgroup w leaves part[2 w] = its min over a, part[2 w + 1] = its max over b
template <class Policy, bool kSame>
__global__ __launch_bounds__(kStreamThreads) void minmax_parts_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t n,
                                                                      float *__restrict__ part) {
    __shared__ float s[8];
    float mn, mx;
    minmax_span<Policy, kSame>(a, b, n, grid_t0(), grid_stride(), &mn, &mx);
    block_minmax(&mn, &mx, s);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = mn;
        part[2 * blockIdx.x + 1] = mx;
    }
}

// the fold of nb partials {min, max}, by every workgroup that needs the result: no launch of its own, no cross-workgroup hand-off
__device__ __forceinline__ void fold_parts(const float *__restrict__ part, int nb, float *mn, float *mx, float *s) {
    float a = INFINITY, b = -INFINITY;
    for (int k = threadIdx.x; k < nb; k += kStreamThreads) {
        a = fminf(a, part[2 * k]);
        b = fmaxf(b, part[2 * k + 1]);
    }
    block_minmax(&a, &b, s);
    *mn = a;
    *mx = b;
}

}  // namespace th
